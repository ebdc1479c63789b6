"""rt_scene_create_albedo and rt_denoise_albedo_device (rt_denoise_albedo.hip): an albedo scene's render against the CPU oracle's
render of the Python-transformed description, and the albedo-guided à-trous filter against the numpy restatement of its definition
(albedo_helpers), bit for bit — filtered means and display bytes alike.

Frames are those of tests/test_gpu_denoise.py, for the same reasons: 1 x 1, 5 x 3, 17 x 9 (no multiple of the 32 x 8 tile), 70 x 37
and 130 x 66 (strides 16 and 32 reach past both edges; several workgroups each way); K = 1..6 makes the LDS kernels of strides 1 and
2 and the gather kernel of strides 4 .. 32 each the last iteration once.  The synthetic albedo has hard edges, zeros, values below
the floor and above 1, and entries that are not finite.

Quality (numpy restatement on the CPU oracle's frames, defaults, against the oracle's 1024-spp mean under another seed; DESIGN.md
section 5 "Albedo-guided denoise"): on earth at 16 spp the undenoised mean's MSE is 2.411898e-04, the plain filter's 7.325543e-04 and
the guided filter's 2.411898e-04 — the earth under a uniform sky has no Monte Carlo noise at all (every path leaves after one bounce:
frame = albedo x sky exactly), only the anti-aliasing noise that the same-path albedo frame shares, so the guided filter returns the
undenoised mean to within rounding (max |out - m| = 5.6e-16) and "strictly below undenoised" is decided in the last bits.  Guided is
far below plain there (the CPU sweep showed it: asserted), which is what the albedo frame is for."""
import numpy as np
import pytest

import albedo_helpers as ah
import denoise_helpers as dh
import kernel_classes
import scene_cases
from adaptive_helpers import assert_bits

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (17, 9), (70, 37), (130, 66)]
SEED = 11
_frames = {}


def frames(w, h):
    if (w, h) not in _frames:
        S, Q, spp, spp_map = dh.synthetic(w, h, 1000 * w + h)
        A, n_a = ah.synthetic_albedo(w, h, 77 * w + h)
        if w * h >= 15:
            a = A / n_a
            assert not np.isfinite(A).all() and (a == 0.0).any() and (a > 1.0).any()
            assert ((a > 0.0) & (a < ah.DEFAULTS["albedo_floor"])).any(), "no albedo below the floor"
            assert {0, 1, 2} <= set(spp_map.reshape(-1).tolist())
        for x in (S, Q, spp_map, A):
            x.setflags(write=False)
        _frames[(w, h)] = (S, Q, spp, spp_map, A, n_a)
    return _frames[(w, h)]


def on_device(rt, S, Q, spp, A, n_a, spp_map=None, guard=64, **kw):
    """rt_denoise_albedo_device into buffers with guards: (means (h, w, 3), bytes (h, w, 4)); nothing outside them may be written"""
    import torch
    h, w = S.shape[:2]
    n = w * h
    d_s, d_q, d_a = (torch.from_numpy(np.array(x)).cuda() for x in (S, Q, A))  # (copies: the shared frames are read-only)
    d_n = torch.from_numpy(np.array(spp_map, dtype=np.int32)).cuda() if spp_map is not None else None
    fill = float(np.uint64(0x7FF8DEADBEEF0001).view(np.float64))
    d_out = torch.full((8 + 3 * n + 8,), fill, dtype=torch.float64, device="cuda")
    d_b = torch.full((guard + 4 * n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws_bytes = rt.denoise_albedo_workspace_bytes(w, h)
    d_ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    rt.denoise_albedo_device(w, h, d_s.data_ptr(), d_q.data_ptr(), spp, d_a.data_ptr(), n_a, d_out.data_ptr() + 64, d_ws.data_ptr(),
                             d_spp_ptr=d_n.data_ptr() if d_n is not None else 0, d_rgba8_ptr=d_b.data_ptr() + guard,
                             params=rt.denoise_albedo_params(**kw), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, raw, ws = d_out.cpu().numpy(), d_b.cpu().numpy(), d_ws.cpu().numpy()
    assert np.isnan(out[:8]).all() and np.isnan(out[-8:]).all(), "values outside d_mean_out were written"
    assert (raw[:guard] == 0xA5).all() and (raw[guard + 4 * n:] == 0xA5).all(), "bytes outside d_rgba8 were written"
    assert (ws[ws_bytes:] == 0xA5).all(), "bytes behind the workspace were written"
    assert_bits(d_s.cpu().numpy(), S, "d_sum after the call")
    assert_bits(d_q.cpu().numpy(), Q, "d_sum_sq after the call")
    assert_bits(d_a.cpu().numpy(), A, "d_albedo_sum after the call")
    return out[8:-8].reshape(h, w, 3), raw[guard:guard + 4 * n].reshape(h, w, 4)


# ---- the albedo scene's render ----
PARITY = {  # case -> (scene_cases name, overrides, the features the ORIGINAL's kernel has at least)
    "random_balls": ("ragged_random_balls_53x29_4spp", {}, "spheres_solid"),
    "earth": ("earth_ragged_image_80x45_8spp", {}, "spheres_quads_textures"),
    "two_perlin_spheres": ("two_perlin_spheres_80x45_8spp", dict(width=40), "spheres_quads_textures"),
    "cornell_smoke": ("cornell_smoke_64x64_16spp", dict(width=32), "quads_frames_media"),
    "simple_light": ("simple_light_80x45_16spp", dict(width=40), "spheres_quads_textures"),
}
_parity = {}


def parity_case(rt, oracle, case):
    if case not in _parity:
        name, over, _ = PARITY[case]
        hs = scene_cases.build(rt, name, **over)
        alb = ah.AlbedoScene(rt, hs)
        want = oracle.render(alb, rt.render_params(seed=SEED))
        want.setflags(write=False)
        _parity[case] = (hs, alb, want)
    return _parity[case]


@pytest.mark.parametrize("walk", ["RT_WALK_OWN_TREES", "RT_WALK_REFERENCE_ORDER"])
@pytest.mark.parametrize("case", list(PARITY))
def test_an_albedo_scenes_render_is_the_oracles_of_the_transformed_description(rt, oracle, gpu, case, walk):
    hs, alb, want = parity_case(rt, oracle, case)
    p = rt.render_params(seed=SEED)
    original = rt.DeviceScene(hs, walk=getattr(rt, walk))
    original.render(p)
    kernel_of_original = rt.debug_last_kernel()
    ds = rt.DeviceScene(hs, albedo=True, walk=getattr(rt, walk))
    assert ds.albedo
    got = ds.render(p, camera=rt.albedo_camera(hs.camera))
    assert_bits(got, want, f"{case}, {walk}: the albedo scene against the oracle")
    kernel = rt.debug_last_kernel()
    assert kernel == kernel_of_original, (kernel, kernel_of_original)
    if case == "random_balls" and walk == "RT_WALK_OWN_TREES":  # solid colours, metals and glass: the appended SOLID textures do not take it out of the spheres-only class
        assert kernel["features"] == kernel_classes.FEAT["spheres_solid"], kernel
    else:
        assert kernel["features"] & kernel_classes.FEAT[PARITY[case][2]] == kernel_classes.FEAT[PARITY[case][2]], kernel
    # an albedo frame is not the beauty frame, and a miss is the white of the camera it was rendered with
    beauty = original.render(p)
    assert not np.array_equal(got, beauty)
    spp = hs.camera.samples_per_pixel
    a = got.reshape(-1, 3) / spp
    assert np.isfinite(a).all() and a.min() >= 0.0
    if case in ("random_balls", "earth", "two_perlin_spheres"):
        assert (a == 1.0).all(axis=1).any(), "no pixel of pure background"
    if case == "simple_light":
        assert (a > 1.0).any(), "the light that is kept emits (4, 4, 4)"
    # the device scene made from the Python-transformed description is the same scene
    assert_bits(rt.DeviceScene(alb, walk=getattr(rt, walk)).render(p, camera=alb.camera), want, f"{case}, {walk}: the transformed description on the device")


# ---- the filter ----
@pytest.mark.parametrize("k", range(1, 7))
@pytest.mark.parametrize("w, h", SIZES)
def test_the_filter_equals_the_definition_bit_for_bit_on_synthetic_frames(rt, gpu, w, h, k):
    S, Q, spp, spp_map, A, n_a = frames(w, h)
    for what, n_arg, n_map in (("uniform spp", spp, None), ("spp map", 0, spp_map)):
        n = spp if n_map is None else n_map
        want = ah.denoise_albedo(S, Q, n, A, n_a, iterations=k)
        got, rgba = on_device(rt, S, Q, n_arg, A, n_a, n_map, iterations=k)
        assert_bits(got, want, f"{w}x{h}, K = {k}, {what}")
        assert np.array_equal(rgba, dh.display(rt, want)), f"{w}x{h}, K = {k}, {what}: display bytes"
        if w * h >= 15:
            C0, _, valid, a, d = ah.prepare(S, Q, n, A, n_a, ah.DEFAULTS["albedo_floor"])
            assert valid.any() and not valid.all()
            assert np.isfinite(got[valid]).all(), "a valid pixel took a tap that is not valid"
            with np.errstate(all="ignore"):
                m = S / np.broadcast_to(np.asarray(n, dtype=np.float64), (h, w))[:, :, None]
            assert_bits(got[~valid], m[~valid], "a pixel that is not valid is written unchanged")
            assert (got != m)[valid].any(), "the filter changed nothing"


def test_an_albedo_of_one_everywhere_is_rt_denoise_device_bit_for_bit(rt, gpu):
    w, h = 70, 37
    S, Q, spp, spp_map, _, _ = frames(w, h)
    for n_a in (1, 5):
        A = np.full((h, w, 3), float(n_a))
        for n_arg, n_map in ((spp, None), (0, spp_map)):
            got, rgba = on_device(rt, S, Q, n_arg, A, n_a, n_map, iterations=4)
            plain, plain_rgba = rt.denoise(S, Q, n_arg, spp_map=n_map, rgba8=True, iterations=4)
            assert_bits(got, plain, f"A = n_a = {n_a}: rt_denoise_albedo_device against rt_denoise_device")
            assert np.array_equal(rgba, plain_rgba)
    assert not np.array_equal(on_device(rt, S, Q, spp, frames(w, h)[4], frames(w, h)[5])[0], plain, equal_nan=True)


def test_the_parameters_are_honoured(rt, gpu):
    # Two flat halves of EQUAL irradiance (1, 1, 1) and non-zero variance: albedo 0.2 on the left, 0.8 on the right, so the means differ
    # (0.2 / 0.8) but the irradiances do not and the luminance stop e lets taps through.  The step of 0.6 is above sigma_albedo 0.5:
    # ea = 0 for every tap across it — no tap crosses.  One iteration (stride 1) shows it pixel by pixel: when the RIGHT half's moments
    # change, no pixel of the left half moves by a bit — but for the column at the edge, whose 3 x 3 prefilter of the variance (no tap:
    # it takes no stop) reaches across.  With a sigma_albedo above the step the taps at dx = +1, +2 do cross.
    w, h, n = 40, 16, 8
    half = w // 2
    rng = np.random.default_rng(5)
    alb = np.where(np.arange(w)[None, :, None] < half, 0.2, 0.8) * np.ones((h, w, 3))
    irr = 1.0 + 0.2 * rng.standard_normal((n, h, w, 3))
    S, Q = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for s in range(n):
        c = irr[s] * alb
        S, Q = S + c, Q + c * c
    A = alb * 4.0
    S2, Q2 = S.copy(), Q.copy()
    S2[:, half:], Q2[:, half:] = S[:, half:] * 1.5, Q[:, half:] * 2.25
    one, _ = on_device(rt, S, Q, n, A, 4, iterations=1)
    one2, _ = on_device(rt, S2, Q2, n, A, 4, iterations=1)
    assert_bits(one, ah.denoise_albedo(S, Q, n, A, 4, iterations=1), "two halves, K = 1")
    assert_bits(one2[:, :half - 1], one[:, :half - 1], "the left half after the right half's moments changed")
    assert (one2[:, half:] != one[:, half:]).all()
    assert (one != S / n)[:, 2:half - 2].any(axis=2).all(), "a pixel inside a half took no tap"
    wide, _ = on_device(rt, S, Q, n, A, 4, iterations=1, sigma_albedo=2.0)
    wide2, _ = on_device(rt, S2, Q2, n, A, 4, iterations=1, sigma_albedo=2.0)
    assert (wide2[:, half - 2:half - 1] != wide[:, half - 2:half - 1]).any(axis=2).all(), "sigma_albedo = 2 kept the halves apart"
    assert_bits(wide2[:, :half - 2], wide[:, :half - 2], "two columns are as far as a stride-1 tap reaches")
    assert_bits(wide, ah.denoise_albedo(S, Q, n, A, 4, iterations=1, sigma_albedo=2.0), "sigma_albedo = 2")
    # all four iterations: the halves stay their own flat colours, and the irradiance inside a half got smoother
    got, _ = on_device(rt, S, Q, n, A, 4)
    assert_bits(got, ah.denoise_albedo(S, Q, n, A, 4), "two halves, defaults")
    assert np.var(got[:, 2:half - 2] / 0.2) < 0.5 * np.var(S[:, 2:half - 2] / n / 0.2)
    assert abs(got[:, :half].mean() - 0.2) < 0.02 and abs(got[:, half:].mean() - 0.8) < 0.08

    # albedo_floor is the divisor where a = 0: a 1 x 1 frame (one tap, the centre) with A = 0 gives ((9/64 * (m / floor)) / (9/64)) * floor
    S1, Q1 = np.array([[[0.75, 1.5, 2.25]]]), np.array([[[0.3, 0.9, 1.9]]])
    for floor in (0.125, 1e-3, 3.0):
        one, _ = on_device(rt, S1, Q1, 3, np.zeros((1, 1, 3)), 2, iterations=1, albedo_floor=floor)
        m = S1 / 3.0
        wq = 9.0 / 64.0
        assert_bits(one, ((wq * (m / floor)) / wq) * floor, f"albedo_floor = {floor} where a = 0")
        assert_bits(one, ah.denoise_albedo(S1, Q1, 3, np.zeros((1, 1, 3)), 2, iterations=1, albedo_floor=floor), f"albedo_floor = {floor}: numpy")
    # rt.denoise_albedo (upload, run, download) is the same call, with its keywords
    mean, rgba = rt.denoise_albedo(S, Q, n, A, 4, rgba8=True)
    assert_bits(mean, got, "rt.denoise_albedo against rt.denoise_albedo_device")
    assert rgba.shape == (h, w, 4) and np.array_equal(rgba, dh.display(rt, got))
    assert_bits(rt.denoise_albedo(S, Q, n, A, 4, iterations=2, sigma=2.0, sigma_albedo=0.7, albedo_floor=0.3),
                ah.denoise_albedo(S, Q, n, A, 4, iterations=2, sigma=2.0, sigma_albedo=0.7, albedo_floor=0.3), "rt.denoise_albedo(**kw)")


def test_end_to_end_on_earth_the_guided_frame_is_the_definitions_and_closer_to_the_converged_one(rt, gpu):
    """CPU figures (oracle frames, numpy restatement, defaults; MSE against the oracle's 1024-spp mean under seed 77): undenoised
    2.411898327188e-04, plain 7.325543394601e-04, guided 2.411898327188e-04 (see the module docstring: the guided frame is the
    undenoised one to within rounding on this scene, so the first assertion is decided in the last bits)."""
    hs = scene_cases.build(rt, "earth_80x45_8spp", spp=16)
    assert (hs.width, hs.height) == (80, 45)
    ds, da = rt.DeviceScene(hs), rt.DeviceScene(hs, albedo=True)
    p = rt.render_params(seed=5, sample_end=16)
    S, Q = ds.render_moments(p)
    A = da.render(p, camera=rt.albedo_camera(hs.camera)).reshape(S.shape)
    got, rgba = rt.denoise_albedo(S, Q, 16, A, 16, rgba8=True)
    want = ah.denoise_albedo(S, Q, 16, A, 16)
    assert_bits(got, want, "earth 80x45, 16 spp: device against numpy on the device's S, Q and A")
    assert np.array_equal(rgba, dh.display(rt, want))
    plain = rt.denoise(S, Q, 16)
    ref = ds.render(rt.render_params(seed=77, sample_end=1024)).reshape(S.shape) / 1024.0
    mse = [float(np.mean((x - ref) ** 2)) for x in (S / 16.0, plain, got)]
    print(f"MSE against the 1024-spp mean: undenoised {mse[0]:.12e}, plain {mse[1]:.12e}, albedo-guided {mse[2]:.12e} "
          f"(guided - undenoised {mse[2] - mse[0]:.3e})")
    assert mse[2] < mse[1], mse           # the CPU sweep showed it on this case
    assert mse[2] < mse[0], mse


def test_the_albedo_render_the_moments_and_the_filter_on_one_stream_equal_the_blocking_route(rt, gpu):
    import torch
    hs = scene_cases.build(rt, "two_perlin_spheres_80x45_8spp", width=40, spp=6)
    w, h = hs.width, hs.height
    ds, da = rt.DeviceScene(hs), rt.DeviceScene(hs, albedo=True)
    p = rt.render_params(seed=SEED, sample_end=6)
    white = rt.albedo_camera(hs.camera)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream):
        d_s = torch.zeros(3 * w * h, dtype=torch.float64, device="cuda")
        d_q, d_a, d_out = torch.zeros_like(d_s), torch.zeros_like(d_s), torch.zeros_like(d_s)
        d_b = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
        d_ws = torch.empty(rt.denoise_albedo_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        da.render_device(p, d_a.data_ptr(), stream.cuda_stream, camera=white)
        ds.render_moments_device(p, d_s.data_ptr(), d_q.data_ptr(), stream.cuda_stream)
        rt.denoise_albedo_device(w, h, d_s.data_ptr(), d_q.data_ptr(), 6, d_a.data_ptr(), 6, d_out.data_ptr(), d_ws.data_ptr(),
                                 d_rgba8_ptr=d_b.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        got, rgba = d_out.cpu().numpy().reshape(h, w, 3), d_b.cpu().numpy().reshape(h, w, 4)
    S, Q = rt.DeviceScene(hs).render_moments(p)
    A = rt.DeviceScene(hs, albedo=True).render(p, camera=white).reshape(S.shape)
    want, want_rgba = rt.denoise_albedo(S, Q, 6, A, 6, rgba8=True)
    assert_bits(got, want, "one stream, one synchronisation, against the blocking route")
    assert np.array_equal(rgba, want_rgba)
    assert_bits(want, ah.denoise_albedo(S, Q, 6, A, 6), "the blocking route against numpy")
    assert not np.array_equal(want, rt.denoise(S, Q, 6)), "the guide changed nothing on a textured scene"
