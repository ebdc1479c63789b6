"""rt_render_moments[_device] and rt_denoise_device (rt_denoise.hip): the moments of a whole frame against the CPU oracle, and the
variance-guided à-trous filter against the numpy restatement of its definition (denoise_helpers), bit for bit.

The filter is a fixed sequence of f64 + - * / sqrt max, so "equal" means equal as u64, for the filtered means and for the display
bytes.  Synthetic frames are small and chosen for the paths they reach: 1 x 1 (smaller than one tap ring), 5 x 3, 17 x 9 (no multiple
of the 32 x 8 tile), 70 x 37 and 130 x 66 (a stride-16 and a stride-32 reach past both edges; more than one workgroup in each
direction); K = 1..6 runs the LDS kernels of strides 1 and 2 and the gather kernel of strides 4 .. 32, each also as the last iteration.

Quality (Cornell box 64 x 64, 16 spp, defaults, against a 1024-spp mean): with the numpy restatement on the CPU oracle's frames the
denoised frame's mean squared error is 0.281 of the undenoised one's; the end-to-end test prints the device's figures before it
asserts the condition (DESIGN.md section 5 "Denoise")."""
import numpy as np
import pytest

import denoise_helpers as dh
from adaptive_helpers import assert_bits

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (17, 9), (70, 37), (130, 66)]
SEED = 11
_frames, _oracle = {}, {}


def frames(w, h):
    if (w, h) not in _frames:
        S, Q, spp, spp_map = dh.synthetic(w, h, 1000 * w + h)
        if w * h >= 15:
            assert not np.isfinite(S).all() and not np.isfinite(Q).all()
            assert {0, 1, 2} <= set(spp_map.reshape(-1).tolist()) and len(np.unique(spp_map)) > 3
        for a in (S, Q, spp_map):
            a.setflags(write=False)
        _frames[(w, h)] = (S, Q, spp, spp_map)
    return _frames[(w, h)]


def on_device(rt, S, Q, spp, spp_map=None, guard=64, **kw):
    """rt_denoise_device into buffers with guards: (means (h, w, 3), bytes (h, w, 4)); nothing outside either may be written"""
    import torch
    h, w = S.shape[:2]
    n = w * h
    d_s, d_q = torch.from_numpy(np.array(S)).cuda(), torch.from_numpy(np.array(Q)).cuda()  # (copies: the shared frames are read-only)
    d_n = torch.from_numpy(np.array(spp_map, dtype=np.int32)).cuda() if spp_map is not None else None
    fill = float(np.uint64(0x7FF8DEADBEEF0001).view(np.float64))
    d_out = torch.full((8 + 3 * n + 8,), fill, dtype=torch.float64, device="cuda")
    d_b = torch.full((guard + 4 * n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws_bytes = rt.denoise_workspace_bytes(w, h)
    d_ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    rt.denoise_device(w, h, d_s.data_ptr(), d_q.data_ptr(), spp, d_out.data_ptr() + 64, d_ws.data_ptr(),
                      d_spp_ptr=d_n.data_ptr() if d_n is not None else 0, d_rgba8_ptr=d_b.data_ptr() + guard,
                      params=rt.denoise_params(**kw), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, raw, ws = d_out.cpu().numpy(), d_b.cpu().numpy(), d_ws.cpu().numpy()
    assert np.isnan(out[:8]).all() and np.isnan(out[-8:]).all(), "values outside d_mean_out were written"
    assert (raw[:guard] == 0xA5).all() and (raw[guard + 4 * n:] == 0xA5).all(), "bytes outside d_rgba8 were written"
    assert (ws[ws_bytes:] == 0xA5).all(), "bytes behind the workspace were written"
    # the inputs are inputs
    assert_bits(d_s.cpu().numpy(), S, "d_sum after the call")
    assert_bits(d_q.cpu().numpy(), Q, "d_sum_sq after the call")
    return out[8:-8].reshape(h, w, 3), raw[guard:guard + 4 * n].reshape(h, w, 4)


@pytest.mark.parametrize("k", range(1, 7))
@pytest.mark.parametrize("w, h", SIZES)
def test_the_filter_equals_the_definition_bit_for_bit_on_synthetic_moments(rt, gpu, w, h, k):
    S, Q, spp, spp_map = frames(w, h)
    for what, n_arg, n_map in (("uniform spp", spp, None), ("spp map", 0, spp_map)):
        want = dh.denoise(S, Q, spp if n_map is None else n_map, iterations=k)
        got, rgba = on_device(rt, S, Q, n_arg, n_map, iterations=k)
        assert_bits(got, want, f"{w}x{h}, K = {k}, {what}")
        assert np.array_equal(rgba, dh.display(rt, want)), f"{w}x{h}, K = {k}, {what}: display bytes"
        if w * h >= 15:
            valid = dh.prepare(S, Q, spp if n_map is None else n_map)[2]
            assert valid.any() and not valid.all()
            assert (np.isfinite(got[valid])).all(), "a valid pixel took a tap that is not valid"
            moved = (got != dh.prepare(S, Q, spp if n_map is None else n_map)[0])[valid]
            assert moved.any(), "the filter changed nothing"
    # a constant map is the uniform route
    same, same_rgba = on_device(rt, S, Q, 0, np.full((h, w), spp, dtype=np.int32), iterations=k)
    uni, uni_rgba = on_device(rt, S, Q, spp, None, iterations=k)
    assert_bits(same, uni, f"{w}x{h}, K = {k}: a constant spp map against the uniform spp")
    assert np.array_equal(same_rgba, uni_rgba)


def test_the_hard_edge_at_zero_variance_stays_hard_and_other_parameters_are_honoured(rt, gpu):
    w, h = 70, 37
    S, Q, spp, _ = frames(w, h)
    bx, by = w // 3, h // 3
    got, _ = on_device(rt, S, Q, spp)
    # after one iteration: a pixel whose 3 x 3 prefilter lies inside the block has sd = 0, so den = eps and every tap off the block's
    # constant has e = 0; the taps on it give (0.25 * sw) / sw
    one, _ = on_device(rt, S, Q, spp, iterations=1)
    rows, cols = slice(by + 1, by + h // 3 - 1), slice(bx + 1, bx + w // 6 - 1)
    valid = dh.prepare(S, Q, spp)[2][rows, cols]
    assert valid.sum() > 20
    assert (one[rows, cols][valid] == 0.25).all(), "a pixel of zero variance took colour from across the edge"
    assert (one[rows, bx + w // 6 + 1:bx + 2 * (w // 6) - 1][dh.prepare(S, Q, spp)[2][rows, bx + w // 6 + 1:bx + 2 * (w // 6) - 1]] == 0.75).all()
    for kw in (dict(sigma=1.0), dict(sigma=16.0, iterations=3), dict(eps=1e-2, iterations=2)):
        g, rgba = on_device(rt, S, Q, spp, **kw)
        want = dh.denoise(S, Q, spp, **{**dh.DEFAULTS, **kw})
        assert_bits(g, want, str(kw))
        assert np.array_equal(rgba, dh.display(rt, want))
        assert not np.array_equal(g, got, equal_nan=True), f"{kw} changed nothing"
    # rt.denoise (upload, run, download) is the same call
    mean, rgba = rt.denoise(S, Q, spp, rgba8=True)
    assert_bits(mean, got, "rt.denoise against rt.denoise_device")
    assert rgba.shape == (h, w, 4) and np.array_equal(rgba, dh.display(rt, got))
    assert_bits(rt.denoise(S, Q, spp, iterations=2, sigma=2.0), dh.denoise(S, Q, spp, iterations=2, sigma=2.0), "rt.denoise(**kw)")


ORACLE_CASES = {"cornell_16x16": (6, 16, 1.0, (16, 16)), "random_spheres_24x16": (0, 24, 1.5, (24, 16))}


def oracle_moments(rt, oracle, case):
    if case not in _oracle:
        scene, width, aspect, size = ORACLE_CASES[case]
        hs = rt.HostScene(scene, width=width, aspect=aspect, spp=5, depth=8)
        assert (hs.width, hs.height) == size
        colours = dh.oracle_samples(rt, oracle, hs, 5, SEED)
        S, Q = dh.moments(colours, (hs.height, hs.width, 3))
        S2, Q2 = dh.moments(colours[:2], (hs.height, hs.width, 3))
        total = oracle.render(hs, rt.render_params(seed=SEED, sample_end=5)).reshape(S.shape)
        assert_bits(S, total, f"{case}: the oracle's single samples against its sum")
        for a in (S, Q, S2, Q2):
            a.setflags(write=False)
        _oracle[case] = (hs, S, Q, S2, Q2)
    return _oracle[case]


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_the_moments_equal_the_oracles(rt, oracle, gpu, case):
    hs, S, Q, S2, Q2 = oracle_moments(rt, oracle, case)
    ds = rt.DeviceScene(hs)
    s, q = ds.render_moments(rt.render_params(seed=SEED, sample_end=5))
    assert s.shape == q.shape == (hs.height, hs.width, 3)
    assert_bits(s, S, f"{case}: sum against the oracle")
    assert_bits(s.reshape(-1), ds.render(rt.render_params(seed=SEED, sample_end=5)), f"{case}: sum against rt_render")
    assert_bits(q, Q, f"{case}: sum_sq against the in-order sum of the oracle's c * c")
    assert (q != s * s / 5.0).any()
    # [0, 2) then [2, 5) with accumulate is [0, 5)
    a, b = ds.render_moments(rt.render_params(seed=SEED, sample_end=2))
    assert_bits(a, S2, f"{case}: [0, 2) sum")
    assert_bits(b, Q2, f"{case}: [0, 2) sum_sq")
    a2, b2 = ds.render_moments(rt.render_params(seed=SEED, sample_begin=2, sample_end=5, accumulate=True), sum=a, sum_sq=b)
    assert a2 is a and b2 is b
    assert_bits(a, S, f"{case}: [0, 2) then [2, 5) sum")
    assert_bits(b, Q, f"{case}: [0, 2) then [2, 5) sum_sq")
    with pytest.raises(rt.RtError, match="accumulate"):
        ds.render_moments(rt.render_params(seed=SEED, sample_begin=2, sample_end=5, accumulate=True))
    # the render after it is the render before it
    assert_bits(ds.render(rt.render_params(seed=SEED, sample_end=5)).reshape(S.shape), S, f"{case}: rt_render after rt_render_moments")


def test_end_to_end_the_denoised_frame_is_the_definitions_and_closer_to_the_converged_one(rt, gpu):
    hs = rt.HostScene(6, width=64, aspect=1.0, spp=16, depth=8)
    assert (hs.width, hs.height) == (64, 64)
    ds = rt.DeviceScene(hs)
    S, Q = ds.render_moments(rt.render_params(seed=5, sample_end=16))
    got, rgba = rt.denoise(S, Q, 16, rgba8=True)
    want = dh.denoise(S, Q, 16)
    assert_bits(got, want, "Cornell box 64x64, 16 spp: device against numpy on the same S and Q")
    assert np.array_equal(rgba, dh.display(rt, want))
    ref = ds.render(rt.render_params(seed=77, sample_end=1024)).reshape(S.shape) / 1024.0
    mse_noisy, mse_denoised = float(np.mean((S / 16.0 - ref) ** 2)), float(np.mean((got - ref) ** 2))
    print(f"MSE against the 1024-spp mean: 16 spp {mse_noisy:.6e}, denoised {mse_denoised:.6e}, ratio {mse_denoised / mse_noisy:.4f}")
    assert mse_denoised < mse_noisy, (mse_denoised, mse_noisy)


def test_the_adaptive_routes_sums_and_spp_map_denoise_to_the_definition(rt, gpu):
    hs = rt.HostScene(6, width=64, aspect=1.0, spp=64, depth=8)
    ds = rt.DeviceScene(hs)
    S, spp, Q, res = ds.render_adaptive(rt.render_params(seed=5, sample_end=64), min_spp=16, batch_spp=16, rel=0.05)
    assert len(np.unique(spp)) > 1, "every pixel stopped at one count: choose other thresholds"
    got, rgba = rt.denoise(S, Q, 0, spp_map=spp, rgba8=True)
    want = dh.denoise(S, Q, spp)
    assert_bits(got, want, "adaptive sums and spp map: device against numpy")
    assert np.array_equal(rgba, dh.display(rt, want))


def test_a_denoise_enqueued_behind_the_moments_on_one_stream_equals_the_blocking_route(rt, gpu):
    import torch
    hs = rt.HostScene(6, width=40, aspect=40 / 28.5, spp=6, depth=8)
    w, h = hs.width, hs.height
    assert (w, h) == (40, 28)
    ds = rt.DeviceScene(hs)
    p = rt.render_params(seed=SEED, sample_end=6)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream):
        d_s = torch.zeros(3 * w * h, dtype=torch.float64, device="cuda")
        d_q = torch.zeros_like(d_s)
        d_out = torch.zeros_like(d_s)
        d_b = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
        d_ws = torch.empty(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        ds.render_moments_device(p, d_s.data_ptr(), d_q.data_ptr(), stream.cuda_stream)
        rt.denoise_device(w, h, d_s.data_ptr(), d_q.data_ptr(), 6, d_out.data_ptr(), d_ws.data_ptr(), d_rgba8_ptr=d_b.data_ptr(),
                          stream=stream.cuda_stream)
        stream.synchronize()
        got, rgba = d_out.cpu().numpy().reshape(h, w, 3), d_b.cpu().numpy().reshape(h, w, 4)
    S, Q = rt.DeviceScene(hs).render_moments(p)
    want, want_rgba = rt.denoise(S, Q, 6, rgba8=True)
    assert_bits(got, want, "one stream, one synchronisation, against the blocking route")
    assert np.array_equal(rgba, want_rgba)
    assert_bits(want, dh.denoise(S, Q, 6), "the blocking route against numpy")
