"""Full-size properties on the GPU: most of BASELINE.json's configurations are too big for the CPU oracle, so at those sizes
the renderer is held to properties that do not depend on size and that the oracle-checked small cases share with
them: the frame is a pure function of (scene, camera, seed) — invariant to how tiles are sharded, to how the
sample range is cut, to where the scene tables live (LDS or global memory) — and additive over sample ranges.
The two configurations the oracle can finish in about a minute of the box's host cores — C2, the one the metric is quoted on,
and C3 — are also compared with it directly, in full (all five: tools/full_config_parity.py, profiles/r03_full_config_parity.txt)."""
import hashlib

import numpy as np
import pytest
import torch

import scene_cases

pytestmark = pytest.mark.gpu
EARTH_LARGE = str(scene_cases.ASSETS / "earth-large.jpg")  # the reference's 6400x3200 asset (assets/README.md)


def digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def render(rt, ds, hs, **kw):
    out = torch.zeros(hs.width * hs.height * 3, dtype=torch.float64, device="cuda")
    ds.render_device(rt.render_params(seed=1, **kw), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def reassemble(rt, ds, hs, shards):
    w, h = hs.width, hs.height
    stride = rt.out_size(w, h, rt.RT_OUT_TILES, 0, shards)
    gathered = torch.zeros(shards * stride, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for r in range(shards):
        ds.render_device(rt.render_params(seed=1, shard_index=r, shard_count=shards, out_layout=rt.RT_OUT_TILES),
                         gathered[r * stride:].data_ptr(), stream)
    frame = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    rt.tiles_to_frame_device(w, h, shards, gathered.data_ptr(), frame.data_ptr(), stream)
    torch.cuda.synchronize()
    return frame


@pytest.mark.parametrize("scene, width, aspect, spp, depth", [(0, 1200, 1.5, 500, 50), (6, 600, 1.0, 1000, 50)], ids=["c2", "c3"])
def test_whole_configuration_equals_the_oracle(rt, gpu, oracle, scene, width, aspect, spp, depth):
    """BASELINE.json configs[1] (random-spheres 1200x800, 500 spp, depth 50: 480 M samples) and configs[2] (Cornell box 600x600, 1000
    spp, depth 50), every sample of every pixel: the GPU's f64 sums against the oracle's, bit for bit.  The oracle runs with the
    narrowing box test — the same image as the reference's own test bit for bit (tests/test_gpu_parity.py: tight == loose), three to four times
    faster: about a minute of 16 host cores for C2."""
    hs = rt.HostScene(scene, scene_seed=1, width=width, aspect=aspect, spp=spp, depth=depth)
    params = rt.render_params(seed=1)
    got = rt.DeviceScene(hs).render(params)
    want = oracle.render(hs, params, aabb_mode=oracle.ORC_AABB_TIGHT)
    assert got.size == hs.width * hs.height * 3
    assert int((got.view(np.uint64) != want.view(np.uint64)).sum()) == 0


def test_c2_random_spheres_1200x800_500spp_depth50(rt, gpu):
    """BASELINE.json configs[1], the bench workload, at its full size."""
    hs = rt.HostScene(0, scene_seed=1, width=1200, aspect=1.5, spp=500, depth=50)
    assert (hs.width, hs.height) == (1200, 800)
    ds = rt.DeviceScene(hs)
    whole = render(rt, ds, hs)
    ref = digest(whole)
    assert digest(render(rt, ds, hs)) == ref                                   # repeatable
    assert digest(reassemble(rt, ds, hs, 8)) == ref                            # 8 tile shards (the 8-GPU partition)
    assert digest(reassemble(rt, ds, hs, 3)) == ref
    # sample ranges chain: [0,137) then [137,500) continuing the sums
    part = render(rt, ds, hs, sample_end=137)
    ds.render_device(rt.render_params(seed=1, sample_begin=137, sample_end=500, accumulate=True), part.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert digest(part) == ref
    # the same frame when the scene is gathered from global memory instead of the LDS (different kernel instantiation)
    assert digest(render(rt, rt.DeviceScene(hs, use_lds=0), hs)) == ref
    # ... and under any scheduler setting (per-scene options: rt_scene_options.th_*)
    assert digest(render(rt, rt.DeviceScene(hs, th_prim=4, th_other=8, th_shade=60, th_box=40, th_new=20), hs)) == ref
    # sanity of the content: a sky-lit scene, every pixel finite and lit, mean radiance per sample in a sane band
    f = whole.cpu().numpy().reshape(800, 1200, 3) / 500.0
    assert np.isfinite(f).all() and f.min() > 0.0 and 0.2 < f.mean() < 0.9
    assert (f[:40].mean(axis=(0, 1)) > np.array([0.5, 0.6, 0.8])).all()       # top rows see mostly sky (0.7, 0.8, 1.0)


def test_c3_cornell_600x600_1000spp_depth50(rt, gpu):
    hs = rt.HostScene(6, scene_seed=1, width=600, aspect=1.0, spp=1000, depth=50)
    ds = rt.DeviceScene(hs)
    whole = render(rt, ds, hs)
    ref = digest(whole)
    assert digest(reassemble(rt, ds, hs, 4)) == ref
    half = render(rt, ds, hs, sample_end=500)
    rest = render(rt, ds, hs, sample_begin=500)
    # disjoint sample ranges are independent estimates: both halves converge to the same image
    a = half.cpu().numpy() / 500.0; b = rest.cpu().numpy() / 500.0
    assert abs(a.mean() - b.mean()) < 0.01 * a.mean()
    ds.render_device(rt.render_params(seed=1, sample_begin=500, accumulate=True), half.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert digest(half) == ref
    f = whole.cpu().numpy().reshape(600, 600, 3) / 1000.0
    assert np.isfinite(f).all() and f.min() >= 0.0
    # red wall on the right of the image, green on the left (src/main.rs:355-366 seen from -z)
    assert f[250:350, 560:, 0].mean() > 3 * f[250:350, 560:, 1].mean()
    assert f[250:350, :40, 1].mean() > 2 * f[250:350, :40, 0].mean()


def test_c4_final_scene_800x800_depth40(rt, gpu):
    """BASELINE.json configs[3] at its full image size; 400 of the 5000 spp keep the test to a few seconds
    (cost and every code path are the same per sample)."""
    hs = rt.HostScene(8, scene_seed=1, width=800, aspect=1.0, spp=400, depth=40, earth_image=EARTH_LARGE)
    ds = rt.DeviceScene(hs)
    st = ds.stats()
    assert st["n_media"] == 2 and st["n_instances"] == 1 and st["image_bytes"] == 6400 * 3200 * 3
    whole = render(rt, ds, hs)
    ref = digest(whole)
    assert digest(reassemble(rt, ds, hs, 8)) == ref
    part = render(rt, ds, hs, sample_end=123)
    ds.render_device(rt.render_params(seed=1, sample_begin=123, accumulate=True), part.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert digest(part) == ref
    f = whole.cpu().numpy() / 400.0
    assert np.isfinite(f).all() and f.min() >= 0.0 and 0.05 < f.mean() < 2.0


def test_c5_final_scene_1600x1600_depth50_in_8_shards(rt, gpu):
    """BASELINE.json configs[4]: final_scene 1600x1600 at depth 50, cut into the 8 tile shards of the 8-GPU run; 48 of the
    10000 spp keep it to seconds.  The sample buffer is capped at 64 MiB for this scene, so the whole frame (61 MB per sample
    row) runs one sample per launch and every shard (7.7 MB per row) fills and drains its buffer six times: chunked launches,
    chained sample ranges and the shard layout all have to agree on one frame."""
    hs = rt.HostScene(8, scene_seed=1, width=1600, aspect=1.0, spp=48, depth=50, earth_image=EARTH_LARGE)
    assert (hs.width, hs.height, hs.camera.max_depth) == (1600, 1600, 50)
    ds = rt.DeviceScene(hs)                                     # default sample buffer (2 GiB): 34 spp per launch
    small = rt.DeviceScene(hs, sample_buffer_bytes=64 << 20)    # 1 spp per launch whole, 8 spp per launch per shard
    whole = render(rt, ds, hs)
    ref = digest(whole)
    assert digest(render(rt, small, hs)) == ref
    assert digest(reassemble(rt, small, hs, 8)) == ref
    # chained ranges on top of chunked launches: [0, 5) [5, 31) [31, 48)
    part = render(rt, small, hs, sample_end=5)
    stream = torch.cuda.current_stream().cuda_stream
    small.render_device(rt.render_params(seed=1, sample_begin=5, sample_end=31, accumulate=True), part.data_ptr(), stream)
    small.render_device(rt.render_params(seed=1, sample_begin=31, accumulate=True), part.data_ptr(), stream)
    torch.cuda.synchronize()
    assert digest(part) == ref
    # the reference-order walk renders the same frame (other kernel, other layout)
    assert digest(render(rt, rt.DeviceScene(hs, walk=rt.RT_WALK_REFERENCE_ORDER), hs)) == ref
    f = whole.cpu().numpy() / 48.0
    assert np.isfinite(f).all() and f.min() >= 0.0 and 0.05 < f.mean() < 2.0


# ---- BASELINE.json configs[3] and [4] at their FULL sample counts (3 s and 26 s of GPU time) ---------------------------------------------
def _fixed_block_error(frame_sums, spp, size):
    """final_scene's 12x12 block means against the reference's screenshot (800x800, depth 40: tests/test_reference_pins.py), in the
    blocks no build-time random number reaches; `size` 1600: the frame is averaged 2x2 first."""
    import test_reference_pins as pins
    lin = np.clip(frame_sums.reshape(size, size, 3) / spp, 0.0, 0.999 ** 2.2)
    if size == 1600:
        lin = lin.reshape(800, 2, 800, 2, 3).mean(axis=(1, 3))
    want = np.asarray(pins.GOLD["shots"]["final_scene"]["blocks_linear"])
    rel = (pins.block_means(lin, pins.GOLD["grid"]) - want) / (want + 0.01)
    fixed = pins.final_scene_fixed_blocks()
    return float(np.abs(rel[fixed]).max()), float(np.sqrt((rel[fixed] ** 2).mean()))


def test_c4_final_scene_800x800_5000spp_depth40_in_full(rt, gpu):
    """The whole of configs[3] — which is also the reference's own final_scene setting (src/main.rs:624-636: 800x800, depth 40), so the
    converged frame has to reproduce the screenshot wherever the scene has no build-time randomness; and the frame is the sum of its two
    halves of the sample range (25 chunked launches each), bit for bit."""
    hs = rt.HostScene(8, scene_seed=1, width=800, aspect=1.0, spp=5000, depth=40, earth_image=EARTH_LARGE)
    ds = rt.DeviceScene(hs)
    whole = render(rt, ds, hs)
    part = render(rt, ds, hs, sample_end=2500)
    ds.render_device(rt.render_params(seed=1, sample_begin=2500, accumulate=True), part.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert digest(part) == digest(whole)
    worst, rms = _fixed_block_error(whole.cpu().numpy(), 5000, 800)
    assert worst < 0.05 and rms < 0.015, (worst, rms)


def test_c5_final_scene_1600x1600_10000spp_depth50_in_full(rt, gpu):
    """The whole of configs[4] on one GPU (26 s), and shard 3 of the 8-GPU partition at full spp (3 s): the shard's tiles are the whole
    frame's, bit for bit; the frame, averaged 2x2, agrees with the reference's 800x800 screenshot in the fixed blocks (depth 50 against
    the screenshot's 40: the extra bounces carry well under a per cent of the light)."""
    hs = rt.HostScene(8, scene_seed=1, width=1600, aspect=1.0, spp=10000, depth=50, earth_image=EARTH_LARGE)
    ds = rt.DeviceScene(hs)
    whole = render(rt, ds, hs)
    f = whole.cpu().numpy()
    assert np.isfinite(f).all() and f.min() >= 0.0
    n = rt.out_size(1600, 1600, rt.RT_OUT_TILES, 3, 8)
    tiles = torch.zeros(n, dtype=torch.float64, device="cuda")
    ds.render_device(rt.render_params(seed=1, shard_index=3, shard_count=8, out_layout=rt.RT_OUT_TILES), tiles.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t = tiles.cpu().numpy().reshape(-1, 8, 8, 3)
    frame = f.reshape(1600, 1600, 3)
    for lt in (0, 1, 777, t.shape[0] - 1):
        k = lt * 8 + 3
        y0, x0 = (k // 200) * 8, (k % 200) * 8
        assert np.array_equal(t[lt].view(np.uint64), np.ascontiguousarray(frame[y0:y0 + 8, x0:x0 + 8]).view(np.uint64)), lt
    k = np.arange(t.shape[0]) * 8 + 3
    rows = ((k // 200) * 8)[:, None, None] + np.arange(8)[None, :, None]
    cols = ((k % 200) * 8)[:, None, None] + np.arange(8)[None, None, :]
    assert np.array_equal(t.view(np.uint64), np.ascontiguousarray(frame[rows, cols]).view(np.uint64))
    worst, rms = _fixed_block_error(f, 10000, 1600)
    assert worst < 0.06 and rms < 0.02, (worst, rms)


# ---- adaptive sampling at full-frame list sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene, width, aspect, depth, rel, abs_", [(6, 600, 1.0, 50, 0.5, 0.2), (0, 1200, 1.5, 50, 0.15, 5e-3)], ids=["c3", "c2"])
def test_adaptive_render_matches_the_oracle_at_every_pixels_own_spp_at_full_frame_size(rt, gpu, oracle, scene, width, aspect, depth, rel, abs_):
    """The twin of tests/test_gpu_adaptive.py's test at C3's 600x600 and C2's 1200x800 frame (lists of 360 000 and 960 000 entries: two
    and four trips of the compaction's scan loop, survivors lists of every size below), schedule 8 : 8 : 32.  The oracle renders the
    snapshots and the single-sample frames (2 x 31 M samples for C2, narrowing box test: the same image bit for bit).  The thresholds
    were settled on the oracle's sums alone so that every schedule point takes its share — Cornell 89 / 3 / 3 / 4 % of the pixels
    (three quarters of them are black after 8 samples), random-spheres 42 / 15 / 13 / 30 % — and a schedule that degenerates fails.
    Added GPU time, measured on an MI355X: 2 s (C3) and 7 s (C2), most of it the oracle; the decode test below: 0.5 s."""
    from adaptive_helpers import check_adaptive_against_oracle
    hs = rt.HostScene(scene, scene_seed=1, width=width, aspect=aspect, spp=32, depth=depth)
    check_adaptive_against_oracle(rt, oracle, hs, rt.DeviceScene(hs), min_spp=8, batch=8, max_spp=32, rel=rel, abs_=abs_, min_share=0.01,
                                  aabb_mode=oracle.ORC_AABB_TIGHT)


def test_list_decode_at_a_large_odd_frame_equals_the_dense_render(rt, gpu):
    """List mode turns an entry into (i, j) with an exact-reciprocal division by the width (rt_kernel.hip, LIST branch); the dense
    render gets its pixels from the tile arithmetic, which is held to the oracle at full size above.  8191 x 4099 (33.6 M pixels,
    both dimensions odd and no multiple of the tile), one sphere, 1 spp, depth 2: the full tile-order list must give the dense
    frame, and a listed subset — the frame's corners, the ends of several rows, pads — its pixels and nothing else.  Compared on
    the device."""
    from adaptive_helpers import PAD, SENTINEL, tile_order
    w, h = 8191, 4099
    hs = rt.HostScene(2, width=w, aspect=w / (h + 0.5), spp=1, depth=2, earth_image=scene_cases.EARTH_SMALL)
    assert (hs.width, hs.height) == (w, h) and (1 << 24) < w * h < (1 << 26)
    ds = rt.DeviceScene(hs)
    stream = torch.cuda.current_stream().cuda_stream
    want = render(rt, ds, hs)

    def listed(pixels, fill):
        lst = torch.from_numpy(np.ascontiguousarray(pixels, dtype=np.uint32).view(np.int32)).cuda()
        out = torch.full((w * h * 3,), fill, dtype=torch.int64, device="cuda").view(torch.float64)
        ds.render_pixels_device(rt.render_params(seed=1), lst.data_ptr(), len(pixels), out.data_ptr(), 0, stream)
        torch.cuda.synchronize()
        return out

    sentinel = int(SENTINEL.astype(np.int64))
    got = listed(tile_order(w, h), sentinel)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    del got
    rows = np.array([0, 1, 2, 7, 8, 1023, 2048, 2049, h - 9, h - 2, h - 1], dtype=np.int64)
    chosen = np.unique(np.concatenate([[0, w * h - 1], rows * w, rows * w + (w - 1), rows * w + 1, rows * w + (w - 2)]))
    g = np.random.default_rng(5)
    g.shuffle(chosen)
    pixels = np.insert(chosen.astype(np.uint32), g.integers(0, chosen.size, 9), PAD)
    got = listed(pixels, sentinel).view(torch.int64).reshape(w * h, 3)
    idx = torch.from_numpy(chosen).cuda()
    assert torch.equal(got[idx], want.view(torch.int64).reshape(w * h, 3)[idx])
    assert int((got != sentinel).sum()) == 3 * chosen.size, "an unlisted pixel was written"
