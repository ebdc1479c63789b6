"""rt_render_views_moments[_device]: views mode with the sums of squares beside the sums (rt_kernel.hip
sum_view_moments_samples_kernel).  `sum` is held, per view, to the CPU oracle under that view's camera and seed — the frames and
helpers of tests/test_gpu_views.py — and `sum_sq` of view v to what rt_render_moments_device writes as d_sum_sq under (views[v].camera,
seed = views[v].seed), as u64 views of the doubles.  A reference frame is rendered once per (case, view, range) and shared.

The cases: 53x29 at 4 spp in 7 views (edge tiles on two sides, grabs that straddle tiles and views; sentinels behind both buffers);
Cornell 64x64 in 3 views of the 30-point arc on the ordered and the fallback walk; a continuation with `accumulate`; a call that the
sample buffer cuts into several launches (a child process, as tests/test_gpu_views.py and tests/test_gpu_launches.py do it: the
switch is read when the library loads); a NaN-filled sum_sq without accumulate; and rt_render_views_device on the same views."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from adaptive_helpers import SENTINEL, assert_bits, bits, launches_for
from test_gpu_views import C3, CORNELL_ARC, RAGGED, assert_views_equal_oracle, orbit, scene

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
_squares, _scenes = {}, {}


def device_scene(rt, case, **opts):
    key = (case, tuple(sorted(opts.items())))
    if key not in _scenes:
        _scenes[key] = rt.DeviceScene(scene(rt, case), **opts)
    return _scenes[key]


def moments_squares(rt, case, view, **range_kw):
    """d_sum_sq of rt_render_moments_device under exactly this view's camera and seed (cached, read-only)"""
    import torch
    key = (case, bytes(view.camera), int(view.seed), tuple(sorted(range_kw.items())))
    if key not in _squares:
        cam = rt.Camera.from_buffer_copy(bytes(view.camera))
        frame = cam.image_width * cam.image_height * 3
        d_s, d_q = (torch.zeros(frame, dtype=torch.float64, device="cuda") for _ in range(2))
        device_scene(rt, case).render_moments_device(rt.render_params(seed=int(view.seed), **range_kw), d_s.data_ptr(), d_q.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream, camera=cam)
        torch.cuda.synchronize()
        q = d_q.cpu().numpy()
        q.setflags(write=False)
        _squares[key] = q
    return _squares[key]


def assert_squares(rt, case, views, got_sq, what, **range_kw):
    n = len(views)
    got_sq = np.asarray(got_sq).reshape(n, -1)
    for v in range(n):
        assert_bits(got_sq[v], moments_squares(rt, case, views[v], **range_kw), f"{what}: sum_sq of view {v} of {n}")


def render_on_device(ds, rt, views, params_list, extra=1024, fill=None, fill_sq=None):
    """rt_render_views_moments_device, one call per entry of params_list, into two torch buffers of n frames with `extra` doubles behind
    them, pre-filled with the sentinel (or `fill` / `fill_sq`, bit patterns): (sum (n, frame), sum_sq (n, frame), tails, launches)"""
    import torch
    n = len(views)
    frame = views[0].camera.image_width * views[0].camera.image_height * 3
    d_s = torch.full((n * frame + extra,), int(SENTINEL) if fill is None else fill, dtype=torch.int64, device="cuda").view(torch.float64)
    d_q = torch.full((n * frame + extra,), int(SENTINEL) if fill_sq is None else fill_sq, dtype=torch.int64, device="cuda").view(torch.float64)
    launches = []
    for p in params_list:
        ds.render_views_moments_device(p, views, d_s.data_ptr(), d_q.data_ptr(), torch.cuda.current_stream().cuda_stream)
        launches.append(rt.debug_last_launch()["launches"])
    torch.cuda.synchronize()
    s, q = d_s.cpu().numpy(), d_q.cpu().numpy()
    return s[:n * frame].reshape(n, frame), q[:n * frame].reshape(n, frame), (s[n * frame:], q[n * frame:]), launches


def test_ragged_frames_in_seven_views(rt, oracle, gpu):
    hs = scene(rt, RAGGED)
    assert (hs.width, hs.height) == (53, 29)
    views = orbit(rt, hs, 7, 21)  # (tests/test_gpu_views.py's views of this case: their oracle frames are shared)
    ds = device_scene(rt, RAGGED)
    s, q, tails, launches = render_on_device(ds, rt, views, [rt.render_params(seed=999)])  # (params.seed is ignored)
    assert launches == [1]
    assert_views_equal_oracle(rt, oracle, RAGGED, views, s, RAGGED)
    assert_squares(rt, RAGGED, views, q, RAGGED)
    for name, tail in zip(("d_sum", "d_sum_sq"), tails):
        assert tail.size == 1024 and (bits(tail) == SENTINEL).all(), f"the buffer behind the last view of {name} was written"
    assert len({bits(q[v]).tobytes() for v in range(7)}) == 7, "two views have the same squares"
    # the host form is the same call; and a NaN-filled sum_sq (and sum) without accumulate is overwritten, not continued
    hs_s, hs_q = ds.render_views_moments(rt.render_params(), views)
    assert hs_s.shape == hs_q.shape == (7, 29, 53, 3)
    assert_bits(hs_s.reshape(7, -1), s, "rt_render_views_moments: sum")
    assert_bits(hs_q.reshape(7, -1), q, "rt_render_views_moments: sum_sq")
    nan = int(np.float64(np.nan).view(np.int64))
    s2, q2, _, _ = render_on_device(ds, rt, views, [rt.render_params()], fill=nan, fill_sq=nan)
    assert_bits(s2, s, "sum over a NaN-filled buffer, accumulate 0")
    assert_bits(q2, q, "sum_sq over a NaN-filled buffer, accumulate 0")
    # rt_render_views_device on the same views still gives sum's bits
    assert_bits(ds.render_views(rt.render_params(), views).reshape(7, -1), s, "rt_render_views_device against the moments call's sum")


@pytest.mark.parametrize("walk", ["own trees, four children", "own trees, two children", "reference order"])
def test_cornell_in_three_views_of_the_arc_on_every_walk(rt, oracle, gpu, walk):
    opts = {"own trees, four children": dict(walk=rt.RT_WALK_OWN_TREES, wide=1), "own trees, two children": dict(walk=rt.RT_WALK_OWN_TREES, wide=0),
            "reference order": dict(walk=rt.RT_WALK_REFERENCE_ORDER)}[walk]
    hs = scene(rt, C3)
    views = list(orbit(rt, hs, 5, 11, CORNELL_ARC))[:3]  # (tests/test_gpu_views.py's views: their oracle frames are shared)
    s, q, _, launches = render_on_device(device_scene(rt, C3, **opts), rt, views, [rt.render_params()])
    assert launches == [1]
    kernel = rt.debug_last_kernel()
    assert bool(kernel["ordered"]) == (walk != "reference order"), kernel
    assert_views_equal_oracle(rt, oracle, C3, views, s, f"{C3}, {walk}")
    assert_squares(rt, C3, views, q, f"{C3}, {walk}")


def test_a_continuation_equals_the_whole_range_in_both_buffers(rt, oracle, gpu):
    hs = scene(rt, RAGGED)
    assert hs.camera.samples_per_pixel == 4
    views = orbit(rt, hs, 7, 21)
    ds = device_scene(rt, RAGGED)
    whole_s, whole_q, _, _ = render_on_device(ds, rt, views, [rt.render_params(sample_begin=0, sample_end=4)])
    split_s, split_q, tails, _ = render_on_device(ds, rt, views, [rt.render_params(sample_begin=0, sample_end=2),
                                                                  rt.render_params(sample_begin=2, sample_end=4, accumulate=True)])
    assert_bits(split_s, whole_s, "[0, 2) + [2, 4) against [0, 4): sum")
    assert_bits(split_q, whole_q, "[0, 2) + [2, 4) against [0, 4): sum_sq")
    assert all((bits(t) == SENTINEL).all() for t in tails)
    assert_views_equal_oracle(rt, oracle, RAGGED, views, whole_s, "[0, 4)")
    assert_squares(rt, RAGGED, views, whole_q, "[0, 4)")
    half_s, half_q, _, _ = render_on_device(ds, rt, views, [rt.render_params(sample_begin=0, sample_end=2)])
    assert (bits(half_q) != bits(whole_q)).any() and (bits(half_s) != bits(whole_s)).any(), "the second range added nothing"
    # the host form continues the arrays it is given
    a, b = ds.render_views_moments(rt.render_params(sample_begin=0, sample_end=2), views)
    ds.render_views_moments(rt.render_params(sample_begin=2, sample_end=4, accumulate=True), views, sum=a, sum_sq=b)
    assert_bits(a.reshape(7, -1), whole_s, "rt_render_views_moments with accumulate: sum")
    assert_bits(b.reshape(7, -1), whole_q, "rt_render_views_moments with accumulate: sum_sq")
    with pytest.raises(rt.RtError):
        ds.render_views_moments(rt.render_params(accumulate=True), views)


CHILD = r"""
import importlib, json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import scene_cases
rt = importlib.import_module("rust-tracing_amd")
case, out, n_views, seed0, spp, of = sys.argv[2], sys.argv[3], *map(int, sys.argv[4:8])
hs = scene_cases.build(rt, case)
views = rt.orbit_views(hs, n_views, seed0, of)
s, q = rt.DeviceScene(hs).render_views_moments(rt.render_params(sample_end=spp), views)
np.save(out + ".sum.npy", s)
np.save(out + ".sq.npy", q)
print(json.dumps({"launches": rt.debug_last_launch()["launches"]}))
"""


@pytest.mark.parametrize("overlap", [0, 1])
def test_a_call_of_several_launches_gives_one_launchs_bits(rt, oracle, gpu, tmp_path, overlap):
    """tests/test_gpu_views.py's route: 5 views of Cornell 64x64 at 9 spp under a 1 MiB sample buffer, a sample row being 480 KiB.  The
    child renders; the parent holds its launch count to the chunk arithmetic and both buffers to this process's one-launch render."""
    n_views, spp, seed0, budget = 5, 9, 71, 1 << 20
    hs = scene(rt, C3)
    want_launches = launches_for(n_views * 64 * 64, spp, budget, overlap)[0]
    assert want_launches >= 3
    out = str(tmp_path / "child")
    env = dict(os.environ, RT_SAMPLE_BUFFER_MB="1", RT_OVERLAP=str(overlap))
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), C3, out, str(n_views), str(seed0), str(spp), str(CORNELL_ARC)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert json.loads(r.stdout.strip().splitlines()[-1])["launches"] == want_launches
    views = orbit(rt, hs, n_views, seed0, CORNELL_ARC)
    one_s, one_q, _, launches = render_on_device(device_scene(rt, C3), rt, views, [rt.render_params(sample_end=spp)])
    assert launches == [1]
    got_s, got_q = np.load(out + ".sum.npy").reshape(n_views, -1), np.load(out + ".sq.npy").reshape(n_views, -1)
    assert_bits(got_s, one_s, f"{want_launches} launches against one, RT_OVERLAP={overlap}: sum")
    assert_bits(got_q, one_q, f"{want_launches} launches against one, RT_OVERLAP={overlap}: sum_sq")
    assert_views_equal_oracle(rt, oracle, C3, views, got_s, f"several launches, RT_OVERLAP={overlap}", sample_end=spp)
    assert_squares(rt, C3, views, got_q, f"several launches, RT_OVERLAP={overlap}", sample_end=spp)
