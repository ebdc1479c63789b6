"""The film stage on the device (rt_film_device) against its host mirror rth_film, bit for bit: every format under every operator at the
sizes where a block ends and the reduction tree changes shape, the three input forms and the encoders' edge table; auto-exposure through
the tone-mapping stage's reduction and workspace; what the call must leave alone; and a real render in the three formats."""
from fractions import Fraction

import numpy as np
import pytest

import film_helpers as fh
import tonemap_helpers as th

pytestmark = pytest.mark.gpu

CURVES = [(th.CLAMP, th.INF), (th.REINHARD, th.INF), (th.REINHARD, 4.0), (th.ACES, th.INF)]
CURVE_IDS = ["clamp", "reinhard", "reinhard-white4", "aces"]
SIZES = [(1, 1), (63, 1), (65, 3)] + [s for s in th.SIZES if s != (1, 1)]
CANARY = 64   # bytes behind d_out that the call must not touch


def _run(rt, values, spp, fmt, *, spp_map=None, stream=None, **kw):
    """one rt_film_device call on uploaded buffers: (the frame as film_host returns it, the values as the device holds them afterwards,
    the workspace's four doubles, the canary bytes behind the output)"""
    import torch
    values = np.array(values, dtype=np.float64)   # (a copy: the shared frames are read-only)
    h, w = values.shape[:2]
    n = rt.film_bytes(w, h, fmt)
    params = rt.tonemap_params(**kw)
    d_values = torch.from_numpy(values).cuda()
    d_spp = torch.from_numpy(np.ascontiguousarray(spp_map, dtype=np.int32)).cuda() if spp_map is not None else None
    d_out = torch.full((n + CANARY,), 0x5A, dtype=torch.uint8, device="cuda")
    d_ws = torch.zeros(rt.tonemap_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream()
    rt.film_device(w, h, d_values.data_ptr(), int(spp), fmt, d_out.data_ptr(), d_spp_ptr=d_spp.data_ptr() if d_spp is not None else 0,
                   d_workspace_ptr=d_ws.data_ptr(), params=params, stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    tail, dtype = {fh.RGBE: ((4,), np.uint8), fh.F32: ((3,), np.uint32), fh.RGB16: ((3,), np.uint16)}[fmt]
    return raw[:n].view(dtype).reshape((h, w) + tail), d_values.cpu().numpy(), d_ws[:32].cpu().numpy().view(np.float64), raw[n:]


@pytest.fixture(scope="module")
def frames():
    out = {("values",) + s: th.value_frame(*s, shift=s[0]) for s in SIZES}
    out[("radiance", 257, 255)] = th.radiance_frame(257, 255, seed=512)
    out[("radiance", 65537, 1)] = th.radiance_frame(65537, 1, seed=65538)
    out[("radiance", 1, 1)] = th.radiance_frame(1, 1, seed=2)
    out[("edges",)] = fh.edge_frame()
    for f in out.values():
        f.setflags(write=False)
    return out


def _host(rt, f, spp, fmt, **kw):
    return fh.as_bits(fmt, rt.film_host(f, spp, fmt, **kw))


@pytest.mark.parametrize("fmt", fh.FORMATS, ids=lambda f: fh.FORMAT_NAMES[f])
@pytest.mark.parametrize("curve", CURVES, ids=CURVE_IDS)
def test_device_frames_are_the_mirrors(rt, gpu, frames, fmt, curve):
    op, white = curve
    for key, f in frames.items():
        kw = dict(op=op, exposure=1.7, white=white)
        got, after, _, canary = _run(rt, f, 1, fmt, **kw)                                  # means
        assert np.array_equal(got, _host(rt, f, 1, fmt, **kw)), key
        assert np.array_equal(after.view(np.uint64), f.view(np.uint64)), "the call must leave d_values untouched"
        assert (canary == 0x5A).all(), "the call must not write behind rt_film_bytes"
    for key in (("values", 257, 255), ("values", 65, 3), ("edges",)):
        f = frames[key]
        h, w = f.shape[:2]
        kw = dict(op=op, exposure=0.5, white=white)
        got, _, _, canary = _run(rt, f, 3, fmt, **kw)                                      # sums with a uniform count
        assert np.array_equal(got, _host(rt, f, 3, fmt, **kw)) and (canary == 0x5A).all(), key
        spp_map = th.spp_map_for(w, h)                                                     # sums with a map
        got, _, _, canary = _run(rt, f, 1, fmt, spp_map=spp_map, **kw)
        assert np.array_equal(got, _host(rt, f, 1, fmt, spp_map=spp_map, **kw)) and (canary == 0x5A).all(), key
    f = frames[("values", 65, 3)]
    got = rt.film(f.copy(), 3, fh.FORMAT_NAMES[fmt], op=op, exposure=0.5, white=white)     # (the upload-run-download wrapper)
    assert np.array_equal(fh.as_bits(fmt, got), _host(rt, f, 3, fmt, op=op, exposure=0.5, white=white))
    assert np.array_equal(_host(rt, frames[("edges",)], 1, fmt, op=op, exposure=1.7, white=white),
                          fh.expected(fmt, frames[("edges",)], 1, op=op, scale=1.7, white=white))   # and the mirror is the definition


@pytest.mark.parametrize("fmt", fh.FORMATS, ids=lambda f: fh.FORMAT_NAMES[f])
def test_auto_exposure_leaves_the_tone_mapping_stages_four_doubles(rt, gpu, frames, fmt):
    import torch
    for key in (("radiance", 257, 255), ("radiance", 65537, 1), ("radiance", 1, 1)):
        f = frames[key]
        h, w = f.shape[:2]
        kw = dict(op="aces", exposure=1.5, auto_key=0.18)
        got, after, out4, canary = _run(rt, f, 1, fmt, **kw)
        d_values = torch.from_numpy(np.array(f)).cuda()                                    # rt_tonemap_device on the same frame and params
        d_rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        d_ws = torch.zeros(rt.tonemap_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        rt.tonemap_device(w, h, d_values.data_ptr(), 1, d_rgb8_ptr=d_rgb.data_ptr(), d_workspace_ptr=d_ws.data_ptr(), params=rt.tonemap_params(**kw),
                          stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        tone4 = d_ws[:32].cpu().numpy().view(np.float64)
        assert [x.hex() for x in out4.tolist()] == [x.hex() for x in tone4.tolist()], key
        assert out4[3] > 0 and out4[2] >= 1
        fixed, _, _, _ = _run(rt, f, 1, fmt, op="aces", exposure=float(out4[3]))           # the bytes follow from that scale
        assert np.array_equal(got, fixed) and np.array_equal(got, _host(rt, f, 1, fmt, **kw)), key
        assert np.array_equal(after.view(np.uint64), f.view(np.uint64)) and (canary == 0x5A).all(), key


def test_another_stream_and_no_workspace(rt, gpu, frames):
    import torch
    f = frames[("values", 257, 255)]
    side = torch.cuda.Stream()
    for fmt in fh.FORMATS:
        got, _, _, canary = _run(rt, f, 1, fmt, stream=side, op="reinhard", exposure=2.0)
        assert np.array_equal(got, _host(rt, f, 1, fmt, op="reinhard", exposure=2.0)) and (canary == 0x5A).all()
    d_values = torch.from_numpy(np.array(frames[("values", 65, 3)])).cuda()                # auto_key == 0: a null workspace is fine
    d_out = torch.zeros(rt.film_bytes(65, 3, "rgbe"), dtype=torch.uint8, device="cuda")
    rt.film_device(65, 3, d_values.data_ptr(), 1, "rgbe", d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().reshape(3, 65, 4), rt.film_host(frames[("values", 65, 3)], 1, "rgbe"))


def test_a_real_render_in_the_three_formats(rt, gpu):
    import torch
    hs = rt.HostScene(5, scene_seed=1, width=24, aspect=1.5, spp=12, depth=8)   # simple_light: an emitter of radiance 4
    assert (hs.width, hs.height) == (24, 16)
    w, h = 24, 16
    sums = rt.DeviceScene(hs, device=0).render(rt.render_params(seed=3)).reshape(h, w, 3)
    assert sums.max() / 12 > 1.0, "the frame must hold radiance above 1"
    # RGB16: the high bytes are rt_tonemap_device's RGB8
    d_sums = torch.from_numpy(np.ascontiguousarray(sums)).cuda()
    d_rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    rt.tonemap_device(w, h, d_sums.data_ptr(), 12, d_rgb8_ptr=d_rgb.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rgb16, _, _, _ = _run(rt, sums, 12, fh.RGB16)
    assert np.array_equal(rgb16 >> 8, d_rgb.cpu().numpy()) and len(np.unique(rgb16)) > 64
    # RGBE: the decoded pixel brackets sums / 12 within the exact bound, and holds what lies above 1
    rgbe, _, _, _ = _run(rt, sums, 12, fh.RGBE)
    m = sums * (1.0 / 12)
    c = fh.rgbe_channel(m)
    lo, hi = fh.rgbe_decode_bounds(rgbe)
    live = rgbe[..., 3] > 0
    assert live.any() and (lo[live] <= c[live]).all() and (c[live] < hi[live]).all()
    assert (rgbe[~live] == 0).all() and all(v < Fraction(2) ** -128 for v in c[~live].ravel())   # the zero pixel only where it belongs
    assert max(lo.ravel()) > 1
    # F32: the means, rounded
    f32, _, _, _ = _run(rt, sums, 12, fh.F32)
    assert np.array_equal(f32, m.astype(np.float32).view(np.uint32)) and f32.view(np.float32).max() > 1.0
