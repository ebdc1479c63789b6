"""rt_scene_create_surface_ids and rt_denoise_guided_device (rt_denoise.hip, the edges and albedo + edges modes): a surface-ID scene's
render against the CPU oracle's render of the Python-transformed description, and the edge-guided à-trous filter against the numpy
restatement of its definition (guided_helpers), bit for bit — filtered means and display bytes alike.

Frames: 1 x 1, 3 x 2, 37 x 19 and 70 x 21 cross the 32 x 8 tile on both axes with ragged edges (several workgroups each way at the
larger two); K = 1 makes the stride-1 LDS kernel the last iteration, K = 4 runs both LDS strides and the gather kernel at strides 4
and 8, the last of them writing the output.  The synthetic guide has blocks of palette colours, anti-aliased borders between them
(0 < eg < 1), a strip of background and entries that are not finite; the moments and the albedo are those of the other filters'
tests."""
import numpy as np
import pytest

import albedo_helpers as ah
import denoise_helpers as dh
import guided_helpers as gh
import kernel_classes
import scene_cases
from adaptive_helpers import assert_bits

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (37, 19), (70, 21)]
SEED = 11
_frames = {}


def frames(w, h):
    if (w, h) not in _frames:
        S, Q, spp, spp_map = dh.synthetic(w, h, 1000 * w + h)
        A, n_a = ah.synthetic_albedo(w, h, 77 * w + h)
        E, n_e = gh.synthetic_edges(w, h, 31 * w + h)
        if w * h >= 15:
            assert not np.isfinite(A).all() and not np.isfinite(E).all() and not np.isfinite(S).all() and not np.isfinite(Q).all()
            assert {0, 1, 2} <= set(spp_map.reshape(-1).tolist())
            g = E / n_e
            assert len({tuple(c) for c in g[np.isfinite(g).all(axis=2)].tolist()}) > 8
        for x in (S, Q, spp_map, A, E):
            x.setflags(write=False)
        _frames[(w, h)] = (S, Q, spp, spp_map, A, n_a, E, n_e)
    return _frames[(w, h)]


def on_device(rt, S, Q, spp, E, n_e, A=None, n_a=0, spp_map=None, guard=64, **kw):
    """rt_denoise_guided_device into buffers with guards: (means (h, w, 3), bytes (h, w, 4)); nothing outside them may be written"""
    import torch
    h, w = S.shape[:2]
    n = w * h
    d_s, d_q, d_e = (torch.from_numpy(np.array(x)).cuda() for x in (S, Q, E))  # (copies: the shared frames are read-only)
    d_a = torch.from_numpy(np.array(A)).cuda() if A is not None else None
    d_n = torch.from_numpy(np.array(spp_map, dtype=np.int32)).cuda() if spp_map is not None else None
    fill = float(np.uint64(0x7FF8DEADBEEF0001).view(np.float64))
    d_out = torch.full((8 + 3 * n + 8,), fill, dtype=torch.float64, device="cuda")
    d_b = torch.full((guard + 4 * n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws_bytes = rt.denoise_guided_workspace_bytes(w, h, A is not None)
    d_ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    rt.denoise_guided_device(w, h, d_s.data_ptr(), d_q.data_ptr(), spp, d_a.data_ptr() if d_a is not None else 0, n_a, d_e.data_ptr(), n_e,
                             d_out.data_ptr() + 64, d_ws.data_ptr(), d_spp_ptr=d_n.data_ptr() if d_n is not None else 0,
                             d_rgba8_ptr=d_b.data_ptr() + guard, params=rt.denoise_guided_params(**kw),
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, raw, ws = d_out.cpu().numpy(), d_b.cpu().numpy(), d_ws.cpu().numpy()
    assert np.isnan(out[:8]).all() and np.isnan(out[-8:]).all(), "values outside d_mean_out were written"
    assert (raw[:guard] == 0xA5).all() and (raw[guard + 4 * n:] == 0xA5).all(), "bytes outside d_rgba8 were written"
    assert (ws[ws_bytes:] == 0xA5).all(), "bytes behind the workspace were written"
    assert_bits(d_s.cpu().numpy(), S, "d_sum after the call")
    assert_bits(d_q.cpu().numpy(), Q, "d_sum_sq after the call")
    assert_bits(d_e.cpu().numpy(), E, "d_edge_sum after the call")
    if A is not None:
        assert_bits(d_a.cpu().numpy(), A, "d_albedo_sum after the call")
    return out[8:-8].reshape(h, w, 3), raw[guard:guard + 4 * n].reshape(h, w, 4)


# ---- the surface-ID scene's render ----
PARITY = {  # case -> (scene_cases name, overrides, the features the ID scene's kernel has at least)
    "cornell_box": ("ragged_cornell_37x37_4spp", {}, "quads_frames"),
    "bouncing_spheres": ("ragged_random_balls_53x29_4spp", {}, "spheres_solid"),
    "cornell_smoke": ("cornell_smoke_64x64_16spp", dict(width=32), "quads_frames_media"),
    "earth": ("earth_ragged_image_80x45_8spp", {}, "spheres_solid"),
}
_parity = {}


def parity_case(rt, oracle, case):
    if case not in _parity:
        name, over, _ = PARITY[case]
        hs = scene_cases.build(rt, name, **over)
        ids = gh.SurfaceIdScene(rt, hs)
        want = oracle.render(ids, rt.render_params(seed=SEED))
        want.setflags(write=False)
        _parity[case] = (hs, ids, want)
    return _parity[case]


@pytest.mark.parametrize("walk", ["RT_WALK_OWN_TREES", "RT_WALK_REFERENCE_ORDER"])
@pytest.mark.parametrize("case", list(PARITY))
def test_an_id_scenes_render_is_the_oracles_of_the_transformed_description(rt, oracle, gpu, case, walk):
    hs, ids, want = parity_case(rt, oracle, case)
    p = rt.render_params(seed=SEED)
    ds = rt.DeviceScene(hs, surface_ids=True, walk=getattr(rt, walk))
    assert ds.surface_ids and not ds.albedo
    black = rt.surface_id_camera(hs.camera)
    assert tuple(black.background.tuple()) == (0.0, 0.0, 0.0)
    got = ds.render(p, camera=black)
    assert_bits(got, want, f"{case}, {walk}: the ID scene against the oracle")
    kernel = rt.debug_last_kernel()
    feat = kernel_classes.FEAT[PARITY[case][2]]
    assert kernel["features"] & feat == feat, kernel
    if case == "earth" and walk == "RT_WALK_OWN_TREES":  # the image texture became a solid: the ID scene left the textured class
        assert kernel["features"] == kernel_classes.FEAT["spheres_solid"], kernel
    if case == "bouncing_spheres":
        assert any(hs.desc.spheres[i].is_moving for i in range(hs.desc.n_spheres)), "no moving centre"
    # an ID frame is not the beauty frame, and every channel of a mean lies in the palette's range
    assert not np.array_equal(got, rt.DeviceScene(hs, walk=getattr(rt, walk)).render(p))
    g = got.reshape(-1, 3) / hs.camera.samples_per_pixel
    assert g.min() >= 0.0 and g.max() <= 1.0
    # the device scene made from the Python-transformed description is the same scene
    assert_bits(rt.DeviceScene(ids, walk=getattr(rt, walk)).render(p, camera=ids.camera), want, f"{case}, {walk}: the transformed description on the device")


@pytest.mark.parametrize("case", list(PARITY))
def test_at_one_sample_every_pixel_is_a_palette_colour_or_the_background(rt, gpu, case):
    name, over, _ = PARITY[case]
    hs = scene_cases.build(rt, name, **over)
    got = rt.DeviceScene(hs, surface_ids=True).render(rt.render_params(seed=3, sample_end=1), camera=rt.surface_id_camera(hs.camera))
    colours = {tuple(c) for c in got.reshape(-1, 3).tolist()}
    allowed = {gh.palette(q) for q in range(1, 27)} | {(0.0, 0.0, 0.0)}
    assert colours <= allowed, colours - allowed
    assert len(colours) >= (2 if case == "earth" else 4), colours
    if case == "cornell_smoke":
        d = hs.desc
        assert {gh.palette((d.n_spheres + d.n_quads + i) % 26 + 1) for i in range(d.n_media)} <= colours, "no path ended inside a medium"


# ---- the filter ----
@pytest.mark.parametrize("with_albedo", [False, True], ids=["edges", "albedo+edges"])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("w, h", SIZES)
def test_the_filter_equals_the_definition_bit_for_bit_on_synthetic_frames(rt, gpu, w, h, k, with_albedo):
    S, Q, spp, spp_map, A, n_a, E, n_e = frames(w, h)
    alb = A if with_albedo else None
    for what, n_arg, n_map in (("uniform spp", spp, None), ("spp map", 0, spp_map)):
        n = spp if n_map is None else n_map
        want = gh.denoise_guided(S, Q, n, E, n_e, alb, n_a, iterations=k)
        got, rgba = on_device(rt, S, Q, n_arg, E, n_e, alb, n_a, n_map, iterations=k)
        assert_bits(got, want, f"{w}x{h}, K = {k}, {what}")
        assert np.array_equal(rgba, dh.display(rt, want)), f"{w}x{h}, K = {k}, {what}: display bytes"
        if w * h >= 15:
            valid = gh.prepare(S, Q, n, E, n_e, alb, n_a)[2]
            assert valid.any() and not valid.all()
            assert np.isfinite(got[valid]).all(), "a valid pixel took a tap that is not valid"
            with np.errstate(all="ignore"):
                m = S / np.broadcast_to(np.asarray(n, dtype=np.float64), (h, w))[:, :, None]
            assert_bits(got[~valid], m[~valid], "a pixel that is not valid is written unchanged")
            assert (got != m)[valid].any(), "the filter changed nothing"
            other = dh.denoise(S, Q, n, iterations=k) if alb is None else ah.denoise_albedo(S, Q, n, A, n_a, iterations=k)
            assert not np.array_equal(got, other, equal_nan=True), "the edge guide changed nothing"


def test_the_display_bytes_are_rt_resolve_rgba8_device_of_the_output(rt, gpu):
    import torch
    w, h = 37, 19
    S, Q, spp, _, A, n_a, E, n_e = frames(w, h)
    for alb in (None, A):
        got, rgba = on_device(rt, S, Q, spp, E, n_e, alb, n_a)
        d_mean = torch.from_numpy(np.ascontiguousarray(got)).cuda()
        d_b = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
        rt.resolve_rgba8_device(w, h, d_mean.data_ptr(), d_b.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(rgba, d_b.cpu().numpy().reshape(h, w, 4))


def test_a_constant_edge_guide_is_the_other_filters_bit_for_bit(rt, gpu):
    w, h = 70, 21
    S, Q, spp, spp_map, A, n_a, _, _ = frames(w, h)
    for n_e, colour in ((1, (0.0, 0.0, 0.0)), (5, (0.5, 1.0, 0.0))):
        E = np.ascontiguousarray(np.broadcast_to(np.array(colour) * n_e, (h, w, 3)))
        for n_arg, n_map in ((spp, None), (0, spp_map)):
            got, rgba = on_device(rt, S, Q, n_arg, E, n_e, None, 0, n_map)
            plain, plain_rgba = rt.denoise(S, Q, n_arg, spp_map=n_map, rgba8=True)
            assert_bits(got, plain, f"E constant, no albedo frame: rt_denoise_guided_device against rt_denoise_device (n_e = {n_e})")
            assert np.array_equal(rgba, plain_rgba)
            got, rgba = on_device(rt, S, Q, n_arg, E, n_e, A, n_a, n_map)
            guided, guided_rgba = rt.denoise_albedo(S, Q, n_arg, A, n_a, spp_map=n_map, rgba8=True)
            assert_bits(got, guided, f"E constant, an albedo frame: rt_denoise_guided_device against rt_denoise_albedo_device (n_e = {n_e})")
            assert np.array_equal(rgba, guided_rgba)


def test_the_parameters_and_the_python_route_are_honoured(rt, gpu):
    w, h = 37, 19
    S, Q, spp, spp_map, A, n_a, E, n_e = frames(w, h)
    kw = dict(iterations=2, sigma=2.0, eps=1e-4, sigma_edge=0.2)
    got, _ = on_device(rt, S, Q, spp, E, n_e, **kw)
    assert_bits(got, gh.denoise_guided(S, Q, spp, E, n_e, **kw), "edges, other parameters")
    assert not np.array_equal(got, on_device(rt, S, Q, spp, E, n_e, iterations=2, sigma=2.0, eps=1e-4, sigma_edge=0.9)[0], equal_nan=True)
    kw.update(sigma_albedo=0.7, albedo_floor=0.3)
    got, _ = on_device(rt, S, Q, spp, E, n_e, A, n_a, **kw)
    assert_bits(got, gh.denoise_guided(S, Q, spp, E, n_e, A, n_a, **kw), "albedo + edges, other parameters")
    # rt.denoise_guided (upload, run, download) is the same call, with its keywords
    mean, rgba = rt.denoise_guided(S, Q, spp, E, n_e, albedo_sum=A, albedo_spp=n_a, rgba8=True, **kw)
    assert_bits(mean, got, "rt.denoise_guided against rt.denoise_guided_device")
    assert rgba.shape == (h, w, 4) and np.array_equal(rgba, dh.display(rt, got))
    assert_bits(rt.denoise_guided(S, Q, 0, E, n_e, spp_map=spp_map), gh.denoise_guided(S, Q, spp_map, E, n_e), "rt.denoise_guided, an spp map, no albedo")


def test_every_refusal_names_the_field_and_leaves_the_output_untouched(rt, gpu):
    import torch
    w, h = 6, 4
    S, Q, spp, _, A, n_a, E, n_e = frames(37, 19)
    d_s, d_q, d_a, d_e = (torch.from_numpy(np.ascontiguousarray(x[:h, :w])).cuda() for x in (S, Q, A, E))
    fill = float(np.uint64(0x7FF8DEADBEEF0001).view(np.float64))
    d_out = torch.full((3 * w * h,), fill, dtype=torch.float64, device="cuda")
    d_b = torch.full((4 * w * h + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    d_ws = torch.full((rt.denoise_guided_workspace_bytes(w, h, True) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    lib = rt.amd_lib()
    dp, nan = rt.denoise_guided_params, float("nan")
    import ctypes as C

    def call(**kw):
        a = dict(w=w, h=h, s=d_s.data_ptr(), q=d_q.data_ptr(), spp=spp, a=d_a.data_ptr(), aspp=n_a, e=d_e.data_ptr(), espp=n_e, params=None,
                 out=d_out.data_ptr(), rgba=d_b.data_ptr(), ws=d_ws.data_ptr())
        a.update(kw)
        p = a["params"]
        rc = lib.rt_denoise_guided_device(a["w"], a["h"], C.c_void_p(a["s"]), C.c_void_p(a["q"]), a["spp"], None, C.c_void_p(a["a"]), a["aspp"],
                                          C.c_void_p(a["e"]), a["espp"], C.byref(p) if p is not None else None, C.c_void_p(a["out"]),
                                          C.c_void_p(a["rgba"]), C.c_void_p(a["ws"]), None)
        return rc, lib.rt_last_error().decode()

    cases = [(dict(w=0), "width"), (dict(s=None), "d_sum is null"), (dict(q=None), "d_sum_sq is null"), (dict(e=None), "d_edge_sum is null"),
             (dict(a=None, e=None), "d_edge_sum is null"), (dict(out=None), "d_mean_out is null"), (dict(ws=None), "d_workspace is null"),
             (dict(spp=1), "spp"), (dict(aspp=0), "albedo_spp"), (dict(espp=0), "edge_spp"),
             (dict(params=rt.DenoiseGuidedParams(struct_size=44)), "struct_size"), (dict(params=dp(iterations=7)), "iterations"),
             (dict(params=dp(sigma=nan)), "sigma"), (dict(params=dp(eps=0.0)), "eps"), (dict(params=dp(sigma_albedo=0.0)), "sigma_albedo"),
             (dict(params=dp(albedo_floor=nan)), "albedo_floor"), (dict(params=dp(sigma_edge=0.0)), "sigma_edge"), (dict(params=dp(sigma_edge=nan)), "sigma_edge"),
             (dict(out=d_s.data_ptr()), "d_mean_out"), (dict(out=d_a.data_ptr() + 8), "d_albedo_sum"), (dict(out=d_e.data_ptr()), "d_edge_sum"),
             (dict(out=d_e.data_ptr() + 8 * (3 * w * h - 1)), "d_edge_sum"), (dict(rgba=d_b.data_ptr() + 1), "d_rgba8"), (dict(ws=d_ws.data_ptr() + 8), "d_workspace")]
    before = [t.clone() for t in (d_s, d_q, d_a, d_e)]
    for kw, field in cases:
        rc, msg = call(**kw)
        assert rc == -1, (kw, rc, msg)   # RT_ERR_INVALID_ARGUMENT
        assert field in msg and msg.startswith("rt_denoise_guided_device: "), (kw, msg)
    torch.cuda.synchronize()
    assert np.isnan(d_out.cpu().numpy()).all(), "a refused call wrote d_mean_out"
    assert (d_b.cpu().numpy() == 0xA5).all() and (d_ws.cpu().numpy() == 0xA5).all(), "a refused call wrote d_rgba8 or the workspace"
    for t, b in zip((d_s, d_q, d_a, d_e), before):
        assert torch.equal(t.view(torch.int64), b.view(torch.int64)), "a refused call wrote an input"
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert_bits(d_out.cpu().numpy().reshape(h, w, 3), gh.denoise_guided(S[:h, :w], Q[:h, :w], spp, E[:h, :w], n_e, A[:h, :w], n_a), "the call that is fine")


def test_end_to_end_on_the_cornell_box_the_edge_guided_frame_is_the_definitions_and_closer_to_the_converged_one(rt, gpu):
    """The sweep's size (64 x 64, 16 spp) against the library's own 1024-spp seed-77 mean: the quality assertion is "strictly below
    the undenoised frame's MSE".  CPU figures (tools/denoise_edges_sweep.py: oracle frames, numpy restatement, defaults, the same
    seeds; DESIGN.md section 5 "Edge-guided denoise" has the table): undenoised 4.4165e-02, plain 1.2418e-02, edges with the ID frame
    1.2133e-02 at sigma_edge 0.5 (1.2300e-02 at 0.25, 1.2156e-02 at 0.75) — the CPU sweep showed the edge guide below plain on this
    case, by 2.3 %, so that is asserted too."""
    hs = scene_cases.build(rt, "c3_cornell_box_64x64_16spp_d50")
    assert (hs.width, hs.height, hs.camera.samples_per_pixel) == (64, 64, 16)
    ds, di = rt.DeviceScene(hs), rt.DeviceScene(hs, surface_ids=True)
    p = rt.render_params(seed=5, sample_end=16)
    S, Q = ds.render_moments(p)
    E = di.render(p, camera=rt.surface_id_camera(hs.camera)).reshape(S.shape)
    got, rgba = rt.denoise_guided(S, Q, 16, E, 16, rgba8=True)
    want = gh.denoise_guided(S, Q, 16, E, 16)
    assert_bits(got, want, "Cornell box 64x64, 16 spp: device against numpy on the device's S, Q and E")
    assert np.array_equal(rgba, dh.display(rt, want))
    plain = rt.denoise(S, Q, 16)
    assert not np.array_equal(got, plain), "the guide changed nothing on a scene of many surfaces"
    ref = ds.render(rt.render_params(seed=77, sample_end=1024)).reshape(S.shape) / 1024.0
    mse = [float(np.mean((x - ref) ** 2)) for x in (S / 16.0, plain, got)]
    print(f"MSE against the 1024-spp mean: undenoised {mse[0]:.12e}, plain {mse[1]:.12e}, edge-guided {mse[2]:.12e}")
    assert mse[2] < mse[0], mse
    assert mse[2] < mse[1], mse           # the CPU sweep showed it on this case


def test_the_id_render_the_moments_and_the_filter_on_one_stream_equal_the_blocking_route(rt, gpu):
    import torch
    hs = scene_cases.build(rt, "cornell_smoke_64x64_16spp", width=32, spp=6)
    w, h = hs.width, hs.height
    ds, di = rt.DeviceScene(hs), rt.DeviceScene(hs, surface_ids=True)
    p = rt.render_params(seed=SEED, sample_end=6)
    black = rt.surface_id_camera(hs.camera)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream):
        d_s = torch.zeros(3 * w * h, dtype=torch.float64, device="cuda")
        d_q, d_e, d_out = torch.zeros_like(d_s), torch.zeros_like(d_s), torch.zeros_like(d_s)
        d_b = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
        d_ws = torch.empty(rt.denoise_guided_workspace_bytes(w, h, False), dtype=torch.uint8, device="cuda")
        di.render_device(p, d_e.data_ptr(), stream.cuda_stream, camera=black)
        ds.render_moments_device(p, d_s.data_ptr(), d_q.data_ptr(), stream.cuda_stream)
        rt.denoise_guided_device(w, h, d_s.data_ptr(), d_q.data_ptr(), 6, 0, 0, d_e.data_ptr(), 6, d_out.data_ptr(), d_ws.data_ptr(),
                                 d_rgba8_ptr=d_b.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        got, rgba = d_out.cpu().numpy().reshape(h, w, 3), d_b.cpu().numpy().reshape(h, w, 4)
    S, Q = rt.DeviceScene(hs).render_moments(p)
    E = rt.DeviceScene(hs, surface_ids=True).render(p, camera=black).reshape(S.shape)
    want, want_rgba = rt.denoise_guided(S, Q, 6, E, 6, rgba8=True)
    assert_bits(got, want, "one stream, one synchronisation, against the blocking route")
    assert np.array_equal(rgba, want_rgba)
    assert_bits(want, gh.denoise_guided(S, Q, 6, E, 6), "the blocking route against numpy")
