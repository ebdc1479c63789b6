"""rt_denoise_mean_spatial_device / rt_denoise_albedo_mean_spatial_device (rt_denoise.hip denoise_prepare_spatial_kernel<R, Guided>, then the
à-trous kernels as they are): the device held to the numpy restatement of tests/spatial_denoise_helpers.py bit for bit (u64 view).

Frames: 1 x 1, 1 x 7, 7 x 1 and 2 x 2 (narrower than every halo), 31 x 8, 33 x 9 (one column and one row past a 32 x 8 tile) and
70 x 19 (three tiles wide, ragged on both axes); R = 1, 2, 3 and K = 1..5 (both LDS kernels and the global one behind the new prepare).
Inputs are live_denoise_helpers.synthetic_means at n = 1 and synthetic_albedo_mean (magnitudes far below 1e150), with NaN and +-inf
pixels placed at a tile corner, in a halo column and at a frame corner.

End to end (Cornell box 64 x 64, one sample through rt_render_mean_moments_device; guided: two_perlin_spheres 80 x 45): the tests print
the mean squared errors against the library's own 1024-spp mean under seed 77 and assert only that the spatially filtered frame's is
strictly below the unfiltered frame's (DESIGN.md section 5 "Spatial variance": the CPU sweep gives 0.207 against 0.884 and, guided at
R = 1, below the unfiltered frame on the Perlin scene as well)."""
import numpy as np
import pytest

import live_denoise_helpers as ldh
import spatial_denoise_helpers as sdh
from adaptive_helpers import assert_bits

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (31, 8), (33, 9), (70, 19)]
_frames, _want = {}, {}


def frames(w, h):
    """(M, M2 filled with NaN, A): shared, read-only"""
    if (w, h) not in _frames:
        M, _, n = ldh.synthetic_means(w, h, 1000 * w + h, n=1)
        A = np.array(ldh.synthetic_albedo_mean(w, h, 77 * w + h))
        M = np.array(M)
        # not-valid pixels where the tiling can go wrong: the frame's corners, a tile's corner and the column a halo stages
        spots = [(0, 0, np.nan), (h - 1, w - 1, np.inf)]
        if w > 32:
            spots += [(min(7, h - 1), 31, -np.inf), (0, 32, np.nan), (min(8, h - 1), 32, np.inf), (h // 2, 33, np.nan)]
        if w * h >= 64:
            for k, (y, x, bad) in enumerate(spots):
                if x < w:
                    (M if k % 2 == 0 else A)[y, x, k % 3] = bad
        elif w * h >= 4:
            M[0, 0, 1] = np.nan
        assert np.abs(M[np.isfinite(M)]).max() < 1e150 and np.abs(A[np.isfinite(A)]).max() < 1e150
        M2 = np.full_like(M, np.nan)
        for a in (M, M2, A):
            a.setflags(write=False)
        _frames[(w, h)] = (M, M2, A)
    return _frames[(w, h)]


def want(w, h, R, k, guided):
    key = (w, h, R, k, guided)
    if key not in _want:
        M, _, A = frames(w, h)
        out = sdh.denoise_albedo_mean_spatial(M, None, 1, A, window_radius=R, iterations=k) if guided else sdh.denoise_mean_spatial(M, None, 1, window_radius=R, iterations=k)
        out.setflags(write=False)
        _want[key] = out
    return _want[key]


def filter_on_device(rt, M, M2, n, A=None, guard=64, spatial=None, entry="spatial", **kw):
    """the spatial entry point (entry="mean": the means form) into buffers with guards: (means (h, w, 3), bytes (h, w, 4), bytes that
    rt_resolve_rgba8_device gives for the means); M2 None is a null d_m2.  Nothing outside the outputs may be written, and the inputs
    are inputs."""
    import torch
    h, w = M.shape[:2]
    n_pix = w * h
    given = [(M, "d_mean")] + ([(M2, "d_m2")] if M2 is not None else []) + ([(A, "d_albedo_mean")] if A is not None else [])
    d_in = [torch.from_numpy(np.array(a)).cuda() for a, _ in given]
    fill = float(np.uint64(0x7FF8DEADBEEF0001).view(np.float64))
    d_out = torch.full((8 + 3 * n_pix + 8,), fill, dtype=torch.float64, device="cuda")
    d_b = torch.full((guard + 4 * n_pix + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_b2 = torch.zeros(4 * n_pix, dtype=torch.uint8, device="cuda")
    ws_bytes = rt.denoise_workspace_bytes(w, h) if A is None else rt.denoise_albedo_workspace_bytes(w, h)
    d_ws = torch.full((256 + ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    d_mean, d_m2 = d_in[0].data_ptr(), (d_in[1].data_ptr() if M2 is not None else 0)
    common = dict(d_rgba8_ptr=d_b.data_ptr() + guard, stream=stream)
    if entry == "spatial":
        common["spatial"] = spatial
    if A is None:
        fn = rt.denoise_mean_spatial_device if entry == "spatial" else rt.denoise_mean_device
        fn(w, h, d_mean, d_m2, n, d_out.data_ptr() + 64, d_ws.data_ptr() + 256, params=rt.denoise_params(**kw), **common)
    else:
        fn = rt.denoise_albedo_mean_spatial_device if entry == "spatial" else rt.denoise_albedo_mean_device
        fn(w, h, d_mean, d_m2, n, d_in[-1].data_ptr(), d_out.data_ptr() + 64, d_ws.data_ptr() + 256, params=rt.denoise_albedo_params(**kw), **common)
    rt.resolve_rgba8_device(w, h, d_out.data_ptr() + 64, d_b2.data_ptr(), stream)
    torch.cuda.synchronize()
    out, raw, ws = d_out.cpu().numpy(), d_b.cpu().numpy(), d_ws.cpu().numpy()
    assert np.isnan(out[:8]).all() and np.isnan(out[-8:]).all(), "values outside d_mean_out were written"
    assert (raw[:guard] == 0xA5).all() and (raw[guard + 4 * n_pix:] == 0xA5).all(), "bytes outside d_rgba8 were written"
    assert (ws[:256] == 0xA5).all() and (ws[256 + ws_bytes:] == 0xA5).all(), "bytes around the workspace were written"
    for got, (a, name) in zip(d_in, given):
        assert_bits(got.cpu().numpy(), a, f"{name} after the call")
    return out[8:-8].reshape(h, w, 3), raw[guard:guard + 4 * n_pix].reshape(h, w, 4), d_b2.cpu().numpy().reshape(h, w, 4)


def test_the_frames_hold_what_the_docstring_says():
    for w, h in SIZES:
        M, M2, A = frames(w, h)
        assert np.isnan(M2).all()
        if w * h >= 4:
            assert not np.isfinite(M).all()
    M, _, A = frames(70, 19)
    assert not np.isfinite(M[7, 31]).all() and not np.isfinite(A[0, 32]).all() and not np.isfinite(M[8, 32]).all() and not np.isfinite(M[0, 0]).all()
    assert (A[np.isfinite(A)] < 1e-3).any() and (A[np.isfinite(A)] > 1.0).any()


@pytest.mark.parametrize("k", range(1, 6))
@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("w, h", SIZES)
def test_the_spatial_route_equals_the_definition_bit_for_bit(rt, gpu, w, h, R, k):
    M, M2, A = frames(w, h)
    sp = rt.denoise_spatial_params(window_radius=R)
    for guided in (False, True):
        expect = want(w, h, R, k, guided)
        got, rgba, resolved = filter_on_device(rt, M, None, 1, A if guided else None, spatial=sp, iterations=k)
        assert_bits(got, expect, f"{w}x{h}, R = {R}, K = {k}, guided = {guided}")
        assert np.array_equal(rgba, resolved), "display bytes against rt_resolve_rgba8_device of the output"
        assert np.array_equal(rgba, sdh.display(rt, expect))
        valid = np.isfinite(M).all(axis=2) & (np.isfinite(A).all(axis=2) if guided else True)
        assert_bits(got[~valid], M[~valid], "a pixel that is not valid comes out unchanged")
        assert np.isfinite(got[valid]).all(), "a valid pixel took a member or a tap that is not valid"
        if w * h >= 64:
            assert not valid.all() and (got != M)[valid].any(), "the filter changed nothing"


@pytest.mark.parametrize("w, h", [(2, 2), (33, 9), (70, 19)])
def test_identities_of_the_route_choice(rt, gpu, w, h):
    M, M2nan, A = frames(w, h)
    rng = np.random.default_rng(w * h)
    M2 = rng.random(M.shape) * 0.1
    for R in (1, 2, 3):
        sp = rt.denoise_spatial_params(window_radius=R)
        # guided with albedo 1 everywhere is the plain spatial route
        plain, plain_b, _ = filter_on_device(rt, M, None, 1, spatial=sp)
        same, same_b, _ = filter_on_device(rt, M, None, 1, np.ones_like(M), spatial=sp)
        assert_bits(same, plain, f"{w}x{h}, R = {R}: albedo mean 1 everywhere against the plain spatial route")
        assert np.array_equal(same_b, plain_b)
        # below the threshold d_m2 is not read: null, NaN-filled and real M2 give the same bytes
        for A_ in (None, A):
            a = filter_on_device(rt, M, None, 1, A_, spatial=sp)
            b = filter_on_device(rt, M, M2nan, 1, A_, spatial=sp)
            c = filter_on_device(rt, M, M2, 1, A_, spatial=sp)
            assert_bits(a[0], b[0], "null d_m2 against NaN-filled d_m2")
            assert_bits(a[0], c[0], "null d_m2 against a real one")
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])
    # at or above the threshold the call is the means form's
    for A_ in (None, A):
        for n, below in ((2, 2), (3, 2), (5, 5), (1, 1), (4, 1)):
            sp = rt.denoise_spatial_params(spatial_below=below, window_radius=3)
            got = filter_on_device(rt, M, M2, n, A_, spatial=sp)
            ref = filter_on_device(rt, M, M2, n, A_, entry="mean")
            assert_bits(got[0], ref[0], f"{w}x{h}: samples = {n}, spatial_below = {below} against the means form")
            assert np.array_equal(got[1], ref[1])
            if n == 1:
                assert_bits(got[0], M, "spatial_below = 1 at one sample: the output is the input")
        # and a threshold above the default takes the spatial route at more samples
        sp = rt.denoise_spatial_params(spatial_below=5)
        got = filter_on_device(rt, M, None, 4, A_, spatial=sp)
        assert_bits(got[0], want(w, h, 1, 4, A_ is not None), f"{w}x{h}: samples = 4 below spatial_below = 5")
    # NULL spatial params are the defaults
    assert_bits(filter_on_device(rt, M, None, 1, spatial=None)[0], want(w, h, 1, 4, False), "spatial = NULL")


def test_other_parameters_are_honoured_and_the_blocking_wrappers_are_the_same_calls(rt, gpu):
    w, h = 70, 19
    M, _, A = frames(w, h)
    kw = dict(iterations=2, sigma=2.0, eps=1e-3)
    got, rgba, _ = filter_on_device(rt, M, None, 1, spatial=rt.denoise_spatial_params(window_radius=2), **kw)
    assert_bits(got, sdh.denoise_mean_spatial(M, None, 1, window_radius=2, **kw), str(kw))
    gkw = dict(iterations=2, sigma=2.0, eps=1e-3, sigma_albedo=0.1, albedo_floor=0.05)
    got_g, _, _ = filter_on_device(rt, M, None, 1, A, spatial=rt.denoise_spatial_params(window_radius=2), **gkw)
    assert_bits(got_g, sdh.denoise_albedo_mean_spatial(M, None, 1, A, window_radius=2, **gkw), str(gkw))
    mean, b = rt.denoise_mean_spatial(M, None, 1, rgba8=True, window_radius=2, **kw)
    assert_bits(mean, got, "rt.denoise_mean_spatial against the device form")
    assert b.shape == (h, w, 4) and np.array_equal(b, rgba)
    assert_bits(rt.denoise_albedo_mean_spatial(M, None, 1, A, window_radius=2, **gkw), got_g, "rt.denoise_albedo_mean_spatial")
    M2 = np.full_like(M, 0.01)
    assert_bits(rt.denoise_mean_spatial(M, M2, 3), ldh.denoise_mean(M, M2, 3), "rt.denoise_mean_spatial above the threshold")
    with pytest.raises(rt.RtError, match="d_m2 is null"):
        rt.denoise_mean_spatial(M, None, 2)


def _mse_case(rt, case, size, guided):
    import torch
    import scene_cases
    hs = scene_cases.build(rt, case)   # the CPU sweep's scene (tools/denoise_spatial_sweep.py)
    w, h = hs.width, hs.height
    assert (w, h) == size
    ds = rt.DeviceScene(hs)
    stream = torch.cuda.current_stream().cuda_stream
    d_mean, d_m2, d_shown, d_same = (torch.full((3 * w * h,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4))
    ws_bytes = rt.denoise_albedo_workspace_bytes(w, h) if guided else rt.denoise_workspace_bytes(w, h)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    p = rt.render_params(seed=5, sample_begin=0, sample_end=1)
    ds.render_mean_moments_device(p, d_mean.data_ptr(), d_m2.data_ptr(), 0, stream)
    albedo = None
    if guided:
        albedo = rt.DeviceScene(hs, albedo=True).render_mean(p, camera=rt.albedo_camera(hs.camera))
        d_alb = torch.from_numpy(np.ascontiguousarray(albedo)).cuda()
        rt.denoise_albedo_mean_spatial_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), 1, d_alb.data_ptr(), d_shown.data_ptr(), d_ws.data_ptr(), stream=stream)
        rt.denoise_albedo_mean_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), 1, d_alb.data_ptr(), d_same.data_ptr(), d_ws.data_ptr(), stream=stream)
    else:
        rt.denoise_mean_spatial_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), 1, d_shown.data_ptr(), d_ws.data_ptr(), stream=stream)
        rt.denoise_mean_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), 1, d_same.data_ptr(), d_ws.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    mean, shown, same = (d.cpu().numpy().reshape(h, w, 3) for d in (d_mean, d_shown, d_same))
    assert_bits(same, mean, "one sample through the means form: the output is the input")      # what the spatial route is for
    expect = sdh.denoise_albedo_mean_spatial(mean, None, 1, albedo) if guided else sdh.denoise_mean_spatial(mean, None, 1)
    assert_bits(shown, expect, "the spatially filtered frame against numpy on the same mean")
    assert not np.array_equal(shown, mean), "the spatial route changed nothing"
    ref = ds.render(rt.render_params(seed=77, sample_end=1024)).reshape(mean.shape) / 1024.0
    mse_noisy, mse_shown = float(np.mean((mean - ref) ** 2)), float(np.mean((shown - ref) ** 2))
    print(f"MSE against the 1024-spp mean: 1 sample {mse_noisy:.6e}, spatially filtered {mse_shown:.6e}, ratio {mse_shown / mse_noisy:.4f}")
    assert mse_shown < mse_noisy, (mse_shown, mse_noisy)


def test_end_to_end_the_first_live_frame_is_closer_to_the_converged_one(rt, gpu):
    _mse_case(rt, "c3_cornell_box_64x64_16spp_d50", (64, 64), guided=False)


def test_end_to_end_the_guided_first_frame_on_a_textured_scene(rt, gpu):
    _mse_case(rt, "two_perlin_spheres_80x45_8spp", (80, 45), guided=True)
