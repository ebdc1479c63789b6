"""rt_denoise_views_device and rt_denoise_albedo_views_device (rt_denoise.hip with the view on the grid's second dimension): a stack of
frames filtered in one set of launches, every view held bit for bit — filtered means and display bytes — to the numpy restatement of
the single-frame definition (denoise_helpers, albedo_helpers) applied to that view on its own, and to a single-frame call on that view.

Frames are synthetic, no scene.  Sizes: 1 x 1; 33 x 9, one 32 x 8 tile plus one pixel each way; 32 x 8, exactly one tile, so that
every halo pixel a workgroup stages and every out-of-tile tap would land wholly in the neighbouring view if the view's own bounds
were not what stops it; 70 x 19, several workgroups each way.  n_views 1, 2 and 5; K = 1..5, so the LDS kernels of strides 1 and 2
and the gather kernel at strides 4, 8 and 16 — on frames shorter than its reach — are each the last iteration once.

Bleed detection: view v's sample values are offset by 10 v, so neighbouring views are nothing alike; view 3 has every pixel not valid
(NaN sums) and view 2 has pixels that are not valid along its first and last rows and at its four corners.  A tap, halo pixel or window
member taken across a view boundary then shows as a bit difference from the restatement, or as a valid pixel turned NaN.

The launch count (K + 1 whatever n_views is) has no counter to assert it through: rt_debug_last_launch counts render launches.
DESIGN.md section 5 "Views denoise" states it from the code."""
import numpy as np
import pytest

import albedo_helpers as ah
import denoise_helpers as dh
import scene_cases
from adaptive_helpers import assert_bits

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (33, 9), (32, 8), (70, 19)]
N_VIEWS = [1, 2, 5]
KS = range(1, 6)
ALL_INVALID, EDGES_INVALID = 3, 2
_stacks, _want, _single = {}, {}, {}


def stack(w, h):
    """(S, Q, A) as (5, h, w, 3), spp, n_a: read-only; a stack of n < 5 views is its first n"""
    if (w, h) not in _stacks:
        S, Q, A = (np.zeros((5, h, w, 3)) for _ in range(3))
        for v in range(5):
            s, q, spp, _ = dh.synthetic(w, h, 1000 * w + h + 17 * v)
            c = 10.0 * v  # every sample of view v offset by 10 v: S + n c and Q + 2 c S + n c^2
            with np.errstate(all="ignore"):  # (the synthetic frames hold a few NaN and infinite entries)
                S[v], Q[v] = s + spp * c, q + 2.0 * c * s + spp * c * c
            a, n_a = ah.synthetic_albedo(w, h, 77 * w + h + 5 * v)
            A[v] = a * (1.0 + 0.25 * v)
        S[ALL_INVALID] = np.nan
        S[EDGES_INVALID, 0, ::2, 0] = np.nan
        S[EDGES_INVALID, h - 1, 1::2, 1] = np.inf
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            Q[EDGES_INVALID, y, x, 2] = np.nan
        if w * h >= 15:
            for v in (0, 1, 4):
                valid = dh.prepare(S[v], Q[v], spp)[2]
                assert valid.any() and not valid.all()
            assert not dh.prepare(S[ALL_INVALID], Q[ALL_INVALID], spp)[2].any()
            edges = dh.prepare(S[EDGES_INVALID], Q[EDGES_INVALID], spp)[2]
            assert not edges[0, 0] and not edges[0, w - 1] and not edges[h - 1, 0] and not edges[h - 1, w - 1] and edges[1:-1].any()
        for x in (S, Q, A):
            x.setflags(write=False)
        _stacks[(w, h)] = (S, Q, A, spp, n_a)
    return _stacks[(w, h)]


def want(rt, guided, w, h, v, k):
    """the restatement's frame of view v on its own, and its display bytes (computed once)"""
    key = (guided, w, h, v, k)
    if key not in _want:
        S, Q, A, spp, n_a = stack(w, h)
        out = ah.denoise_albedo(S[v], Q[v], spp, A[v], n_a, iterations=k) if guided else dh.denoise(S[v], Q[v], spp, iterations=k)
        _want[key] = (out, dh.display(rt, out))
    return _want[key]


def single(rt, guided, w, h, v, k):
    """the single-frame entry point on view v's frames (computed once)"""
    key = (guided, w, h, v, k)
    if key not in _single:
        S, Q, A, spp, n_a = stack(w, h)
        _single[key] = (rt.denoise_albedo(S[v], Q[v], spp, A[v], n_a, rgba8=True, iterations=k) if guided
                        else rt.denoise(S[v], Q[v], spp, rgba8=True, iterations=k))
    return _single[key]


def on_device(rt, guided, S, Q, A, spp, n_a, guard=64, **kw):
    """the views call into buffers with guards: (means (n, h, w, 3), bytes (n, h, w, 4)); nothing outside them may be written, the
    inputs stay as they were"""
    import torch
    n, h, w = S.shape[:3]
    px = n * w * h
    d_s, d_q, d_a = (torch.from_numpy(np.array(x)).cuda() for x in (S, Q, A))  # (copies: the shared frames are read-only)
    fill = float(np.uint64(0x7FF8DEADBEEF0001).view(np.float64))
    d_out = torch.full((8 + 3 * px + 8,), fill, dtype=torch.float64, device="cuda")
    d_b = torch.full((guard + 4 * px + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws_bytes = rt.denoise_albedo_views_workspace_bytes(w, h, n) if guided else rt.denoise_views_workspace_bytes(w, h, n)
    d_ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if guided:
        rt.denoise_albedo_views_device(w, h, n, d_s.data_ptr(), d_q.data_ptr(), spp, d_a.data_ptr(), n_a, d_out.data_ptr() + 64, d_ws.data_ptr(),
                                       d_rgba8_ptr=d_b.data_ptr() + guard, params=rt.denoise_albedo_params(**kw), stream=stream)
    else:
        rt.denoise_views_device(w, h, n, d_s.data_ptr(), d_q.data_ptr(), spp, d_out.data_ptr() + 64, d_ws.data_ptr(),
                                d_rgba8_ptr=d_b.data_ptr() + guard, params=rt.denoise_params(**kw), stream=stream)
    torch.cuda.synchronize()
    out, raw, ws = d_out.cpu().numpy(), d_b.cpu().numpy(), d_ws.cpu().numpy()
    assert np.isnan(out[:8]).all() and np.isnan(out[-8:]).all(), "values outside d_mean_out were written"
    assert (raw[:guard] == 0xA5).all() and (raw[guard + 4 * px:] == 0xA5).all(), "bytes outside d_rgba8 were written"
    assert (ws[ws_bytes:] == 0xA5).all(), "bytes behind the workspace were written"
    assert_bits(d_s.cpu().numpy(), S, "d_sum after the call")
    assert_bits(d_q.cpu().numpy(), Q, "d_sum_sq after the call")
    assert_bits(d_a.cpu().numpy(), A, "d_albedo_sum after the call")
    return out[8:-8].reshape(n, h, w, 3), raw[guard:guard + 4 * px].reshape(n, h, w, 4)


@pytest.mark.parametrize("n_views", N_VIEWS)
@pytest.mark.parametrize("w, h", SIZES)
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_every_view_equals_the_definition_and_the_single_frame_call(rt, gpu, guided, w, h, n_views):
    S, Q, A, spp, n_a = stack(w, h)
    for k in KS:
        got, rgba = on_device(rt, guided, S[:n_views], Q[:n_views], A[:n_views], spp, n_a, iterations=k)
        for v in range(n_views):
            what = f"{'guided' if guided else 'plain'}, {w}x{h}, {n_views} views, K = {k}, view {v}"
            want_mean, want_rgba = want(rt, guided, w, h, v, k)
            assert_bits(got[v], want_mean, f"{what}: against the definition")
            assert np.array_equal(rgba[v], want_rgba), f"{what}: display bytes against the definition"
            one_mean, one_rgba = single(rt, guided, w, h, v, k)
            assert_bits(got[v], one_mean, f"{what}: against the single-frame call")
            assert np.array_equal(rgba[v], one_rgba), f"{what}: display bytes against the single-frame call"
            if w * h >= 15:
                valid = (ah.prepare(S[v], Q[v], spp, A[v], n_a, ah.DEFAULTS["albedo_floor"])[2] if guided else dh.prepare(S[v], Q[v], spp)[2])
                assert np.isfinite(got[v][valid]).all(), f"{what}: a valid pixel took a tap that is not valid"
                with np.errstate(all="ignore"):
                    m = S[v] / float(spp)
                assert_bits(got[v][~valid], m[~valid], f"{what}: a pixel that is not valid is written unchanged")
                if v not in (ALL_INVALID,):
                    assert (got[v] != m)[valid].any(), f"{what}: the filter changed nothing"


def test_the_blocking_wrappers_are_the_same_calls(rt, gpu):
    w, h = 70, 19
    S, Q, A, spp, n_a = stack(w, h)
    mean, rgba = rt.denoise_views(S, Q, spp, rgba8=True)
    assert mean.shape == (5, h, w, 3) and rgba.shape == (5, h, w, 4)
    g_mean, g_rgba = rt.denoise_albedo_views(S, Q, spp, A, n_a, rgba8=True, iterations=3, sigma_albedo=0.7)
    for v in range(5):
        assert_bits(mean[v], want(rt, False, w, h, v, 4)[0], f"rt.denoise_views, view {v}")
        assert np.array_equal(rgba[v], want(rt, False, w, h, v, 4)[1])
        assert_bits(g_mean[v], ah.denoise_albedo(S[v], Q[v], spp, A[v], n_a, iterations=3, sigma_albedo=0.7), f"rt.denoise_albedo_views(**kw), view {v}")
        assert np.array_equal(g_rgba[v], dh.display(rt, g_mean[v]))
    assert_bits(rt.denoise_views(S[:2], Q[:2], spp, iterations=2, sigma=2.0)[1], dh.denoise(S[1], Q[1], spp, iterations=2, sigma=2.0), "rt.denoise_views(**kw)")
    with pytest.raises(rt.RtError):
        rt.denoise_views(S[0], Q[0], spp)


def test_end_to_end_views_moments_into_the_views_filter_equal_the_single_frame_route(rt, gpu):
    """Cornell 64 x 64 at 16 spp in 3 views of the 30-point arc, all on the device and one stream: rt_render_views_moments_device into
    rt_denoise_views_device equals, per view, rt_render_moments into rt_denoise_device byte for byte — which is the quality check: the
    single-frame filter's error bound carries over through the identity."""
    import torch
    hs = scene_cases.build(rt, "c3_cornell_box_64x64_16spp_d50")
    w, h, n, spp = hs.width, hs.height, 3, 16
    assert (w, h, hs.camera.samples_per_pixel) == (64, 64, spp)
    views = list(rt.orbit_views(hs, 5, 11, 30))[:n]
    ds = rt.DeviceScene(hs)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream):
        d_s = torch.zeros(n * 3 * w * h, dtype=torch.float64, device="cuda")
        d_q, d_out = torch.zeros_like(d_s), torch.zeros_like(d_s)
        d_b = torch.zeros(n * 4 * w * h, dtype=torch.uint8, device="cuda")
        d_ws = torch.empty(rt.denoise_views_workspace_bytes(w, h, n), dtype=torch.uint8, device="cuda")
        ds.render_views_moments_device(rt.render_params(), views, d_s.data_ptr(), d_q.data_ptr(), stream.cuda_stream)
        rt.denoise_views_device(w, h, n, d_s.data_ptr(), d_q.data_ptr(), spp, d_out.data_ptr(), d_ws.data_ptr(), d_rgba8_ptr=d_b.data_ptr(),
                                stream=stream.cuda_stream)
        stream.synchronize()
        got, rgba = d_out.cpu().numpy().reshape(n, h, w, 3), d_b.cpu().numpy().reshape(n, h, w, 4)
    for v in range(n):
        cam = rt.Camera.from_buffer_copy(bytes(views[v].camera))
        S, Q = ds.render_moments(rt.render_params(seed=int(views[v].seed)), camera=cam)
        one, one_rgba = rt.denoise(S, Q, spp, rgba8=True)
        assert_bits(got[v], one, f"view {v}: the views route against render_moments -> denoise")
        assert rgba[v].tobytes() == one_rgba.tobytes(), f"view {v}: display bytes"
        assert (got[v] != S / float(spp)).any(), "the filter changed nothing"
    assert len({got[v].tobytes() for v in range(n)}) == n
