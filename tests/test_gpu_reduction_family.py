"""The six kernels that fold a launch's sample buffer into the caller's frame (rt_kernel.hip reduce_samples: sum_samples_kernel,
sum_listed_samples_kernel, sum_view_samples_kernel, sum_view_moments_samples_kernel, mean_samples_kernel, mean_moments_samples_kernel)
are instantiations of one body, so some of their outputs are the same bits by construction.  This file pins those relations between the
forms, GPU against GPU, as u64 views of the doubles; each form is held to the CPU oracle by the route's own test file.

One frame of 20 x 12 pixels (3 x 2 tiles, partial on the right and at the bottom) of the cheapest stock scene, 5 samples, one seed.

Relations that another file already asserts in this form are left out here:
  * render_moments' `sum` equals render's frame: tests/test_gpu_denoise.py::test_the_moments_equal_the_oracles;
  * render_views_moments' `sum` equals render_views' array: tests/test_gpu_views_moments.py::test_ragged_frames_in_seven_views;
  * render_views_moments cut into several launches equals its one-launch bits:
    tests/test_gpu_views_moments.py::test_a_call_of_several_launches_gives_one_launchs_bits.

Measured on an MI355X: the views test takes 0.18 s, the two mean tests 0.02 s together; run alone the file takes 12 s, 11 s of which
is the shards test's first use of torch on the GPU in the process.  Inside the suite an earlier file pays for that, and none of the
four is among the suite's 15 slowest tests (the 15th takes 3.9 s)."""
import numpy as np
import pytest

import scene_cases
from adaptive_helpers import SENTINEL, assert_bits, bits

pytestmark = pytest.mark.gpu

SEED, N = 4, 5
_cache = {}


def host_scene(rt):
    if "hs" not in _cache:
        hs = scene_cases.build(rt, "two_spheres_80x45_8spp", width=20, aspect=20 / 12.5, spp=N)
        assert (hs.width, hs.height) == (20, 12)
        _cache["hs"] = hs
    return _cache["hs"]


def one_launch(rt):
    """(render_mean's (mean, rgba8), render_mean_moments' (mean, m2, rgba8)) from one launch each (cached, read-only)"""
    if "mean" not in _cache:
        ds = rt.DeviceScene(host_scene(rt))
        p = rt.render_params(seed=SEED, sample_end=N)
        plain = ds.render_mean(p, rgba8=True)
        assert rt.debug_last_launch()["launches"] == 1
        moments = ds.render_mean_moments(p, rgba8=True)
        assert rt.debug_last_launch()["launches"] == 1
        for a in plain + moments:
            a.setflags(write=False)
        _cache["mean"] = (plain, moments)
    return _cache["mean"]


def test_each_view_equals_the_dense_render_under_its_camera_and_seed(rt, gpu):
    hs = host_scene(rt)
    ds = rt.DeviceScene(hs)
    views = rt.orbit_views(hs, 2, 31)
    frames = ds.render_views(rt.render_params(sample_end=N), views)
    assert frames.shape == (2, 12, 20, 3)
    for v in range(2):
        cam = rt.Camera.from_buffer_copy(bytes(views[v].camera))
        dense = ds.render(rt.render_params(seed=int(views[v].seed), sample_end=N), camera=cam)
        assert_bits(frames[v].reshape(-1), dense.reshape(-1), f"view {v} against rt_render under its camera and seed")
    assert (bits(frames[0]) != bits(frames[1])).any(), "the two views are one frame"


def test_the_mean_with_moments_is_the_plain_means_frame_and_display(rt, gpu):
    (mean, rgba), (mean_m, m2, rgba_m) = one_launch(rt)
    assert_bits(mean_m, mean, "render_mean_moments' mean against render_mean's")
    assert rgba.dtype == rgba_m.dtype == np.uint8 and rgba.shape == rgba_m.shape == (12, 20, 4)
    assert (rgba == rgba_m).all(), "the two RGBA8 frames differ"
    assert (m2 > 0.0).any() and not (m2 < 0.0).any()


def test_the_mean_pair_in_several_launches_gives_the_one_launch_bits(rt, gpu):
    hs = host_scene(rt)
    (mean, rgba), (mean_m, m2, rgba_m) = one_launch(rt)
    row = ((hs.width + 7) // 8) * ((hs.height + 7) // 8) * 64 * 24  # one sample of every tile (tests/test_gpu_live.py)
    ds = rt.DeviceScene(hs, sample_buffer_bytes=3 * row)
    p = rt.render_params(seed=SEED, sample_end=N)
    got, got_rgba = ds.render_mean(p, rgba8=True)
    launches = rt.debug_last_launch()["launches"]
    assert launches >= 2, launches
    assert_bits(got, mean, f"render_mean in {launches} launches against one")
    assert (got_rgba == rgba).all(), f"render_mean's RGBA8 frame in {launches} launches against one"
    got, got_m2, got_rgba = ds.render_mean_moments(p, rgba8=True)
    launches = rt.debug_last_launch()["launches"]
    assert launches >= 2, launches
    assert_bits(got, mean_m, f"render_mean_moments' mean in {launches} launches against one")
    assert_bits(got_m2, m2, f"render_mean_moments' M2 in {launches} launches against one")
    assert (got_rgba == rgba_m).all(), f"render_mean_moments' RGBA8 frame in {launches} launches against one"


def test_four_shards_in_tiles_layout_zero_their_padding_and_keep_every_pixel(rt, gpu):
    import torch
    hs = host_scene(rt)
    ds = rt.DeviceScene(hs)
    w, h, shards, tiles_x = hs.width, hs.height, 4, 3
    whole = ds.render(rt.render_params(seed=SEED, sample_end=N))
    stride = rt.out_size(w, h, rt.RT_OUT_TILES, 0, shards)
    assert stride == 2 * 64 * 3  # 6 tiles over 4 shards: 2, 2, 1, 1
    gathered = torch.full((shards * stride,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
    stream = torch.cuda.current_stream().cuda_stream
    for r in range(shards):
        ds.render_device(rt.render_params(seed=SEED, sample_end=N, shard_index=r, shard_count=shards, out_layout=rt.RT_OUT_TILES),
                         gathered[r * stride:].data_ptr(), stream)
    frame = torch.full((w * h * 3,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
    rt.tiles_to_frame_device(w, h, shards, gathered.data_ptr(), frame.data_ptr(), stream)
    torch.cuda.synchronize()
    assert_bits(frame.cpu().numpy(), whole.reshape(-1), "4 shards in tiles layout, reassembled, against the one-shard frame")
    got = bits(gathered.cpu().numpy()).reshape(shards, stride // 3, 3)
    n_padding = 0
    for r in range(shards):
        n_local = rt.out_size(w, h, rt.RT_OUT_TILES, r, shards) // (64 * 3)
        assert n_local == (2, 2, 1, 1)[r]
        idx = np.arange(n_local * 64)
        k, p = (idx >> 6) * shards + r, idx & 63
        inside = ((k % tiles_x) * 8 + (p & 7) < w) & ((k // tiles_x) * 8 + (p >> 3) < h)
        assert (got[r, :n_local * 64][~inside] == 0).all(), f"shard {r}: a padding pixel is not +0.0"
        assert (got[r, :n_local * 64][inside] != SENTINEL).all(), f"shard {r}: a pixel of the frame was not written"
        assert (got[r, n_local * 64:] == SENTINEL).all(), f"shard {r}: the buffer behind its last tile was written"
        n_padding += int((~inside).sum())
    assert n_padding == 6 * 64 - w * h
