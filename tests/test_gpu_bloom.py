"""Bloom on the device (rt_bloom_device) against its host mirror and the numpy restatement of include/rt_amd.h "bloom"
(tests/bloom_helpers.py), bit for bit: every listed frame in the three input forms, with each level form — one launch through the LDS,
two global passes — on both sides of every switch-over stride, the identity to the existing output stage's bytes on a real render, and a
second call on a used workspace."""
import numpy as np
import pytest

import bloom_helpers as bh

pytestmark = pytest.mark.gpu

KW = dict(threshold=0.5, strength=0.7)


@pytest.fixture(scope="module")
def cases():
    """per shape: the frame, its spp map, and the restated result of each input form — computed once, never written"""
    out = {}
    for w, h, levels in bh.SHAPES + bh.LONG:
        f, smap = bh.frame(w, h, seed=w + h), bh.spp_map_for(w, h)
        forms = {"sums": (7, None), "map": (1, smap), "means": (1, None)}
        want = {name: bh.bloom(f, spp, m, levels=levels, **KW) for name, (spp, m) in forms.items()}
        for a in (f, smap, *want.values()):
            a.setflags(write=False)
        out[(w, h)] = (f, forms, want, levels)
    return out


@pytest.fixture()
def fused(rt):
    """sets the largest stride that runs as one launch, and puts the built-in choice back afterwards"""
    lib = rt.amd_lib()
    yield lambda max_stride: lib.rt_debug_set_bloom_fused(max_stride)
    lib.rt_debug_set_bloom_fused(-1)


@pytest.mark.parametrize("w,h", [(w, h) for w, h, _ in bh.SHAPES + bh.LONG], ids=lambda v: str(v))
def test_device_bits_are_the_mirrors_and_the_restatements(rt, gpu, cases, w, h):
    f, forms, want, levels = cases[(w, h)]
    for name, (spp, smap) in forms.items():
        got = rt.bloom(f, spp, spp_map=smap, levels=levels, **KW)
        assert bh.same_bits(got, want[name]), (name, int((got.view(np.uint64) != want[name].view(np.uint64)).sum()))
        assert bh.same_bits(got, rt.bloom_host(f, spp, spp_map=smap, levels=levels, **KW)), name


@pytest.mark.parametrize("max_stride", [0, 1, 2])
def test_every_level_form_gives_the_same_bits_at_every_stride(rt, gpu, cases, fused, max_stride):
    """The built-in rule keeps frames this small on the global pair, so the one-launch form is forced.  levels >= 4: strides 1, 2, 4, 8, so
    with max_stride = 0, 1, 2 each fused kernel and the global pair run at the stride below and above every switch-over, and strides 4
    and 8 are always the global pair; K = 1, 2 end on each fused kernel's output form, K = 3 on the global pair's"""
    assert fused(max_stride) == -1, "the built-in rule must have been in force"
    for size in ((65, 17), (17, 9), (130, 70), (256, 8), (8, 256)):
        f, forms, want, levels = cases[size]
        for name in ("sums", "map"):
            spp, smap = forms[name]
            assert bh.same_bits(rt.bloom(f, spp, spp_map=smap, levels=levels, **KW), want[name]), (size, name)
    f = cases[(65, 17)][0]
    for levels in (1, 2, 3):   # the last level's output through every form
        assert bh.same_bits(rt.bloom(f, 7, levels=levels, **KW), bh.bloom(f, 7, levels=levels, **KW)), levels


def test_a_frame_of_many_tiles_takes_the_one_launch_form_by_itself(rt, gpu, fused):
    """1030 x 520 is 17 x 33 = 561 tiles of 64 x 16 pixels, above the 512 from which the built-in rule runs strides 1 and 2 as one launch
    each: the rule's result is the restatement's, and the global pair's"""
    w, h = 1030, 520
    f = bh.frame(w, h, seed=7)
    kw = dict(levels=3, **KW)
    want = bh.bloom(f, 7, **kw)
    got = rt.bloom(f, 7, **kw)
    assert bh.same_bits(got, want), int((got.view(np.uint64) != want.view(np.uint64)).sum())
    fused(0)
    assert bh.same_bits(rt.bloom(f, 7, **kw), want)


def test_no_bright_pixel_then_the_clamp_gives_the_existing_stages_bytes(rt, gpu):
    import torch
    hs = rt.HostScene(5, scene_seed=1, width=32, aspect=4.0 / 3.0, spp=4, depth=8)   # simple_light: an emitter of radiance 4
    assert (hs.width, hs.height) == (32, 24)
    sums = rt.DeviceScene(hs, device=0).render(rt.render_params(seed=3)).reshape(24, 32, 3)
    mean = bh.means(sums, 4)
    assert mean.max() > 1.0 and np.isfinite(mean).all() and not np.signbit(mean[mean == 0.0]).any()
    d_mean = torch.from_numpy(np.ascontiguousarray(mean)).cuda()
    d_old = torch.zeros((24, 32, 4), dtype=torch.uint8, device="cuda")
    rt.resolve_rgba8_device(32, 24, d_mean.data_ptr(), d_old.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    old = d_old.cpu().numpy()
    top = float(bh.luminance(mean).max())
    bloomed = rt.bloom(sums, 4, threshold=top, strength=5.0)          # L > threshold nowhere
    assert bh.same_bits(bloomed, mean)
    _, rgba = rt.tonemap(bloomed, 1, rgba8=True)                      # the clamp, exposure 1, no key
    assert np.array_equal(rgba, old) and len(np.unique(rgba)) > 8
    # and with the default threshold the emitter glows: the bytes beside it change, nothing gets darker
    glow = rt.bloom(sums, 4)
    assert bh.same_bits(glow, bh.bloom(sums, 4)) and (glow >= mean).all() and (glow > mean).any()
    assert not np.array_equal(rt.tonemap(glow, 1, rgba8=True)[1], old)


def test_a_second_call_on_the_same_workspace_gives_the_same_bits(rt, gpu, cases):
    import torch
    f, forms, want, levels = cases[(65, 17)]
    w, h = 65, 17
    stream = torch.cuda.current_stream().cuda_stream
    d_ws = torch.full((rt.bloom_workspace_bytes(w, h),), 0xFF, dtype=torch.uint8, device="cuda")   # (all-ones doubles are NaNs: a stale A would show)
    d_out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    d_other = torch.from_numpy(np.ascontiguousarray(bh.frame(w, h, seed=99, special=False) * 50.0)).cuda()
    d_f = torch.from_numpy(np.array(f)).cuda()
    params = rt.bloom_params(levels=levels, **KW)
    got = []
    for d_values in (d_f, d_other, d_f):   # the second call leaves another frame's B, H and A behind
        rt.bloom_device(w, h, d_values.data_ptr(), 7, d_out.data_ptr(), d_ws.data_ptr(), params=params, stream=stream)
        torch.cuda.synchronize()
        got.append(d_out.cpu().numpy())
    assert bh.same_bits(got[0], want["sums"]) and bh.same_bits(got[2], want["sums"]) and not bh.same_bits(got[1], got[0])
    assert bh.same_bits(d_f.cpu().numpy(), f), "the call must leave d_values untouched"
