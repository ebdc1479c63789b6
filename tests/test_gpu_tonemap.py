"""The tone-mapping stage on the device (rt_tonemap_device, rt_log_average_luminance_device) against its host mirror and the numpy
restatement of include/rt_amd.h "tone mapping" (tests/tonemap_helpers.py), bit for bit: bytes in every input form and output layout, the
clamp identity against the three existing output stages on real renders, the reduction's four doubles at every size where the tree
changes shape, auto-exposure end to end, and a stack of frames as one tall frame."""
import numpy as np
import pytest

import tonemap_helpers as th

pytestmark = pytest.mark.gpu

NAMES = {th.CLAMP: "clamp", th.REINHARD: "reinhard", th.ACES: "aces"}


def _run(rt, values, spp, *, spp_map=None, rgb=True, rgba=True, **kw):
    """one rt_tonemap_device call on uploaded buffers: (rgb8 or None, rgba8 or None, the values as the device holds them afterwards)"""
    import torch
    values = np.array(values, dtype=np.float64)   # (a copy: the shared frames are read-only)
    h, w = values.shape[:2]
    params = rt.tonemap_params(**kw)
    d_values = torch.from_numpy(values).cuda()
    d_spp = torch.from_numpy(np.ascontiguousarray(spp_map, dtype=np.int32)).cuda() if spp_map is not None else None
    d_rgb = torch.full((h, w, 3), 0x5a, dtype=torch.uint8, device="cuda") if rgb else None
    d_rgba = torch.full((h, w, 4), 0x5a, dtype=torch.uint8, device="cuda") if rgba else None
    d_ws = torch.zeros(rt.tonemap_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    rt.tonemap_device(w, h, d_values.data_ptr(), int(spp), d_spp_ptr=d_spp.data_ptr() if d_spp is not None else 0,
                      d_rgb8_ptr=d_rgb.data_ptr() if rgb else 0, d_rgba8_ptr=d_rgba.data_ptr() if rgba else 0, d_workspace_ptr=d_ws.data_ptr(),
                      params=params, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (d_rgb.cpu().numpy() if rgb else None, d_rgba.cpu().numpy() if rgba else None, d_values.cpu().numpy(),
            d_ws[:32].cpu().numpy().view(np.float64))


@pytest.fixture(scope="module")
def frames():
    out = {(w, h): th.value_frame(w, h, shift=w) for w, h in th.SIZES}
    for f in out.values():
        f.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def radiance():
    out = {(w, h): th.radiance_frame(w, h, seed=w + h) for w, h in th.SIZES}
    for f in out.values():
        f.setflags(write=False)
    return out


@pytest.mark.parametrize("op", th.OPS, ids=lambda o: NAMES[o])
@pytest.mark.parametrize("white", [th.INF, 4.0])
def test_device_bytes_are_the_mirrors_and_the_restatements(rt, gpu, frames, op, white):
    for (w, h), f in frames.items():
        kw = dict(op=op, exposure=1.7, white=white)
        want = th.expected_rgb8(f, 1, op=op, scale=1.7, white=white)
        assert np.array_equal(rt.tonemap_host(f, 1, **kw), want), (w, h)
        rgb, rgba, _, _ = _run(rt, f, 1, **kw)                     # means, both outputs in one call
        assert np.array_equal(rgb, want) and np.array_equal(rgba, th.rgba_of(want)), (w, h)
    f = frames[(257, 255)]
    kw = dict(op=op, exposure=0.5, white=white)
    want = th.expected_rgb8(f, 3, op=op, scale=0.5, white=white)  # sums with a uniform count; one output at a time
    assert np.array_equal(rt.tonemap_host(f, 3, **kw), want)
    rgb, none, _, _ = _run(rt, f, 3, rgba=False, **kw)
    assert none is None and np.array_equal(rgb, want)
    none, rgba, _, _ = _run(rt, f, 3, rgb=False, **kw)
    assert none is None and np.array_equal(rgba, th.rgba_of(want))
    spp_map = th.spp_map_for(257, 255)                             # sums with a map
    want = th.expected_rgb8(f, 1, spp_map, op=op, scale=0.5, white=white)
    assert np.array_equal(rt.tonemap_host(f, 1, spp_map=spp_map, **kw), want)
    rgb, rgba, _, _ = _run(rt, f, 1, spp_map=spp_map, **kw)
    assert np.array_equal(rgb, want) and np.array_equal(rgba, th.rgba_of(want))
    assert np.array_equal(rt.tonemap(f.copy(), 1, spp_map=spp_map, **kw), want)  # (the upload-run-download wrapper)


def test_clamp_is_the_three_existing_output_stages_on_real_renders(rt, gpu):
    import torch
    hs = rt.HostScene(5, scene_seed=1, width=24, aspect=1.5, spp=12, depth=8)   # simple_light: an emitter of radiance 4
    assert (hs.width, hs.height) == (24, 16)
    w, h = 24, 16
    ds = rt.DeviceScene(hs, device=0)
    stream = torch.cuda.current_stream().cuda_stream

    sums = ds.render(rt.render_params(seed=3)).reshape(h, w, 3)
    assert sums.max() / 12 > 1.0, "the frame must hold radiance above 1"
    d_sums = torch.from_numpy(np.ascontiguousarray(sums)).cuda()
    d_old = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    rt.resolve_rgb8_device(w, h, 12, d_sums.data_ptr(), d_old.data_ptr(), stream)
    torch.cuda.synchronize()
    plain, _, _, _ = _run(rt, sums, 12)
    assert np.array_equal(plain, d_old.cpu().numpy()) and len(np.unique(plain)) > 8

    asum, aspp, _, _ = ds.render_adaptive(rt.render_params(seed=3), min_spp=4, batch_spp=4, rel=0.05)
    assert aspp.min() < aspp.max()
    d_asum, d_aspp = torch.from_numpy(asum).cuda(), torch.from_numpy(aspp).cuda()
    rt.resolve_rgb8_spp_device(w, h, d_asum.data_ptr(), d_aspp.data_ptr(), d_old.data_ptr(), stream)
    torch.cuda.synchronize()
    rgb, _, _, _ = _run(rt, asum, 1, spp_map=aspp)
    assert np.array_equal(rgb, d_old.cpu().numpy())

    mean, shown = ds.render_mean(rt.render_params(seed=3, sample_end=4), rgba8=True)
    d_mean = torch.from_numpy(mean).cuda()
    d_old4 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    rt.resolve_rgba8_device(w, h, d_mean.data_ptr(), d_old4.data_ptr(), stream)
    torch.cuda.synchronize()
    _, rgba, _, _ = _run(rt, mean, 1)
    assert np.array_equal(rgba, d_old4.cpu().numpy()) and np.array_equal(rgba, shown)
    # and the curve does what the clamp cannot: what it clips flat (the emitter, radiance 4) comes back below white
    clipped = (plain == 255).all(axis=2)
    aces, _, _, _ = _run(rt, sums, 12, op="aces", exposure=0.25)
    assert clipped.any() and (aces[clipped] < 255).all()


def test_the_log_average_is_the_hosts_four_doubles(rt, gpu, radiance):
    for (w, h), f in radiance.items():
        host = rt.log_average_luminance_host(f, 1)
        dev = rt.log_average_luminance(f, 1)
        assert [x.hex() for x in dev] == [x.hex() for x in host], (w, h)
        assert dev[3] == 0.0 and 0 < dev[2] <= w * h
    w, h = 257, 255
    f = radiance[(w, h)]
    spp_map = th.spp_map_for(w, h)
    for kw in (dict(spp=3), dict(spp=1, spp_map=spp_map), dict(spp=1, delta=1e-2)):
        spp = kw.pop("spp")
        assert [x.hex() for x in rt.log_average_luminance(f, spp, **kw)] == [x.hex() for x in rt.log_average_luminance_host(f, spp, **kw)], kw
    want_mean, want_count = th.log_average(f, 1)
    dev = rt.log_average_luminance(f, 1)
    assert (dev[0].hex(), dev[2]) == (float(want_mean).hex(), want_count)
    nothing = np.full((3, 5, 3), float("nan"))
    assert rt.log_average_luminance(nothing, 1) == (0.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("op", th.OPS, ids=lambda o: NAMES[o])
def test_auto_exposure_is_the_fixed_exposure_at_the_hosts_scale(rt, gpu, radiance, op):
    for size in ((257, 255), (65537, 1), (1, 1)):
        f = radiance[size]
        log_mean, lavg, count, _ = rt.log_average_luminance_host(f, 1)
        scale = th.scale_of(1.5, 0.18, lavg, count)
        rgb, rgba, after, out4 = _run(rt, f, 1, op=op, exposure=1.5, auto_key=0.18)
        assert [x.hex() for x in out4.tolist()] == [x.hex() for x in (log_mean, lavg, count, scale)], size
        fixed, fixed4, _, _ = _run(rt, f, 1, op=op, exposure=scale)
        assert np.array_equal(rgb, fixed) and np.array_equal(rgba, fixed4), size
        assert np.array_equal(rgb, rt.tonemap_host(f, 1, op=op, exposure=1.5, auto_key=0.18)), size
        assert np.array_equal(after.view(np.uint64), f.view(np.uint64)), "the call must leave d_values untouched"
    g = th.value_frame(5, 3)
    g[..., 1] = float("nan")   # nothing counts: scale = exposure
    rgb, _, _, out4 = _run(rt, g, 1, op=op, exposure=1.7, auto_key=0.18)
    assert out4.tolist() == [0.0, 0.0, 0.0, 1.7]
    assert np.array_equal(rgb, _run(rt, g, 1, op=op, exposure=1.7)[0])


def test_a_stack_of_frames_is_one_tall_frame_when_auto_is_off(rt, gpu):
    w, h, n = 24, 16, 3
    stack = np.concatenate([th.radiance_frame(w, h, seed=k) * 10.0 ** (k - 1) for k in range(n)], axis=0)
    assert stack.shape == (n * h, w, 3)
    kw = dict(op="aces", exposure=0.7)
    rgb, rgba, _, _ = _run(rt, stack, 1, **kw)
    for k in range(n):
        one, one4, _, _ = _run(rt, stack[k * h:(k + 1) * h], 1, **kw)
        assert np.array_equal(rgb[k * h:(k + 1) * h], one) and np.array_equal(rgba[k * h:(k + 1) * h], one4), k
    # the header's caveat: auto-exposure over the stack pools the views into one log-average
    pooled, _, _, _ = _run(rt, stack, 1, auto_key=0.18, **kw)
    own, _, _, _ = _run(rt, stack[:h], 1, auto_key=0.18, **kw)
    assert not np.array_equal(pooled[:h], own)
