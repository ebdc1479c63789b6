"""The host-memory render entry points against their device twins: rt_render (both layouts, sharded and not, with and without
`accumulate`), rt_render_views with `accumulate`, and rt_render_adaptive with and without the squares.  Every comparison is bit for bit
on the u64 view of the doubles; the expected values are always what the *_device form wrote, so no oracle frame is rendered here.
(rt_render_mean and rt_render_mean_moments are held to the frames their device forms are held to, continuation included, by
test_the_host_buffer_form_gives_the_device_forms_bits of tests/test_gpu_live.py and tests/test_gpu_live_denoise.py.)

The frame is 20 x 12 at 4 spp: 3 x 2 tiles, the right column 4 pixels wide and the bottom row 4 pixels high, so rt_render's scatter from
its tile buffer clips on both edges and in the corner; with shard_count 4 the six tiles split 2, 2, 1, 1.  The scene is random-balls
(the views tests' ragged case, made smaller): below the flat sky of the top rows next to every pixel has a value of its own, and
setup() asserts that no two tiles hold the same values where they overlap, so a tile in the wrong place shows."""
import ctypes as C

import numpy as np
import pytest

import scene_cases
from adaptive_helpers import SENTINEL, assert_bits, bits
from test_gpu_views import RAGGED, orbit

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 20, 12, 4, 5
TILES_X, N_TILES = 3, 6
_made = {}


def setup(rt):
    """(host scene, device scene, the unsharded RT_OUT_FRAME frame of rt_render_device (h, w, 3), read-only), made once"""
    if not _made:
        hs = scene_cases.build(rt, RAGGED, width=W, aspect=W / (H + 0.5), spp=SPP)
        assert (hs.width, hs.height, hs.camera.samples_per_pixel) == (W, H, SPP)
        ds = rt.DeviceScene(hs)
        frame = on_device(rt, ds, rt.render_params(seed=SEED)).reshape(H, W, 3)
        blocks = [frame[(k // TILES_X) * 8:(k // TILES_X) * 8 + 4, (k % TILES_X) * 8:(k % TILES_X) * 8 + 4] for k in range(N_TILES)]
        for a in range(N_TILES):  # (4 x 4: what every tile has inside the frame)
            for b in range(a):
                assert (bits(blocks[a]) != bits(blocks[b])).any(), f"tiles {a} and {b} start with the same values: a misplaced tile could hide"
        frame.setflags(write=False)
        _made.update(hs=hs, ds=ds, frame=frame)
    return _made["hs"], _made["ds"], _made["frame"]


def on_device(rt, ds, p):
    """rt_render_device into a torch buffer of out_size zeros"""
    import torch
    d = torch.zeros(rt.out_size(W, H, p.out_layout, p.shard_index, p.shard_count), dtype=torch.float64, device="cuda")
    ds.render_device(p, d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def shard_mask(index, count):
    """(h, w) bool: the pixels of the shard's tiles, k = local * count + index, row-major over the tiles of a row"""
    mask = np.zeros((H, W), dtype=bool)
    for k in range(index, N_TILES, count):
        x0, y0 = (k % TILES_X) * 8, (k // TILES_X) * 8
        mask[y0:y0 + 8, x0:x0 + 8] = True
    return mask


def filled(n, pattern=SENTINEL):
    return np.full(n, pattern, dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("count", [1, 4])
def test_rt_render_equals_rt_render_device_in_both_layouts_on_every_shard(rt, gpu, count):
    hs, ds, frame = setup(rt)
    sizes = []
    for index in range(count):
        what = f"shard {index} of {count}"
        tiles = rt.render_params(seed=SEED, shard_index=index, shard_count=count, out_layout=rt.RT_OUT_TILES)
        got = ds.render(tiles)
        sizes.append(got.size // (64 * 3))
        assert_bits(got, on_device(rt, ds, tiles), f"{what}: RT_OUT_TILES")
        out = filled(W * H * 3)
        assert ds.render(rt.render_params(seed=SEED, shard_index=index, shard_count=count), out=out) is out
        out, mask = out.reshape(H, W, 3), shard_mask(index, count)
        assert_bits(out[mask], frame[mask], f"{what}: RT_OUT_FRAME, the pixels of its tiles")
        assert (bits(out[~mask]) == SENTINEL).all(), f"{what}: RT_OUT_FRAME wrote a pixel of another shard's tile"
    assert sizes == ([6] if count == 1 else [2, 2, 1, 1])


@pytest.mark.parametrize("layout, index, count", [("RT_OUT_FRAME", 0, 1), ("RT_OUT_FRAME", 1, 4), ("RT_OUT_TILES", 1, 4)])
def test_rt_render_continued_with_accumulate_equals_one_call(rt, gpu, layout, index, count):
    hs, ds, frame = setup(rt)
    common = dict(seed=SEED, shard_index=index, shard_count=count, out_layout=getattr(rt, layout))
    whole = ds.render(rt.render_params(sample_end=SPP, **common))
    out = np.zeros(whole.size)
    ds.render(rt.render_params(sample_end=2, **common), out=out)
    assert (bits(out) != bits(whole)).any(), "two samples already give the four samples' sums"
    ds.render(rt.render_params(sample_begin=2, sample_end=SPP, accumulate=True, **common), out=out)
    assert_bits(out, whole, f"{layout}, shard {index} of {count}: [0, 2) then [2, {SPP})")
    if layout == "RT_OUT_FRAME":
        mask = shard_mask(index, count)
        assert_bits(out.reshape(H, W, 3)[mask], frame[mask], "the shard's pixels against rt_render_device")
        assert (bits(out.reshape(H, W, 3)[~mask]) == 0).all(), "another shard's pixels of the zero frame were written"
    else:
        assert_bits(out, on_device(rt, ds, rt.render_params(sample_end=SPP, **common)), "against rt_render_device")
    with pytest.raises(rt.RtError, match="accumulate"):
        ds.render(rt.render_params(sample_begin=2, sample_end=SPP, accumulate=True, **common))


def test_rt_render_views_continued_with_accumulate_equals_one_call_and_the_device_form(rt, gpu):
    import torch
    hs, ds, _ = setup(rt)
    views = orbit(rt, hs, 2, 17)
    whole = ds.render_views(rt.render_params(sample_end=SPP), views)
    assert whole.shape == (2, H, W, 3)
    out = np.zeros_like(whole)
    ds.render_views(rt.render_params(sample_end=2), views, out=out)
    ds.render_views(rt.render_params(sample_begin=2, sample_end=SPP, accumulate=True), views, out=out)
    assert_bits(out, whole, f"[0, 2) then [2, {SPP})")
    d = torch.from_numpy(filled(whole.size)).cuda()
    ds.render_views_device(rt.render_params(sample_end=SPP), views, d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_bits(whole.reshape(-1), d.cpu().numpy(), "rt_render_views against rt_render_views_device")
    assert (bits(whole[0]) != bits(whole[1])).any(), "the two views rendered the same frame"


def test_rt_render_adaptive_equals_rt_render_adaptive_device_with_and_without_the_squares(rt, gpu):
    """min_spp 2, batches of 2, at most 6 samples: three schedule points, and at least two batches must run"""
    import torch
    hs, ds, _ = setup(rt)
    params = rt.render_params(seed=SEED, sample_end=6)
    a = rt.adaptive_params(min_spp=2, batch_spp=2, rel_threshold=0.05, abs_threshold=1e-3)
    d_sum, d_sq = (torch.from_numpy(filled(W * H * 3)).cuda() for _ in range(2))
    d_spp = torch.full((W * H,), -1, dtype=torch.int32, device="cuda")
    want_res = ds.render_adaptive_device(params, a, d_sum.data_ptr(), d_spp.data_ptr(), d_sq.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert want_res["launches"] >= 2, want_res
    total, spp, sq, res = ds.render_adaptive(params, min_spp=2, batch_spp=2, rel=0.05, abs=1e-3)
    assert_bits(total.reshape(-1), d_sum.cpu().numpy(), "sums")
    assert_bits(sq.reshape(-1), d_sq.cpu().numpy(), "sums of squares")
    assert np.array_equal(spp.reshape(-1), d_spp.cpu().numpy()) and res == want_res
    # without the caller's squares the library keeps them in scratch of its own; the guard behind the sums stays
    buf, spp2, res2 = filled(W * H * 3 + 8), np.full(W * H, -1, dtype=np.int32), rt.AdaptiveResult()
    rc = rt.amd_lib().rt_render_adaptive(ds._handle, C.byref(hs.camera), C.byref(params), C.byref(a), C.c_void_p(buf.ctypes.data),
                                         C.c_void_p(spp2.ctypes.data), None, C.byref(res2))
    assert rc == 0, rt.amd_lib().rt_last_error()
    assert_bits(buf[:-8], total.reshape(-1), "sums without out_rgb_sum_sq")
    assert (bits(buf[-8:]) == SENTINEL).all(), "values behind out_rgb_sum were written"
    assert np.array_equal(spp2, spp.reshape(-1)) and res2.as_dict() == res
