"""rt_render_mean_moments[_device] (rt_kernel.hip mean_moments_samples_kernel) and rt_denoise_mean_device /
rt_denoise_albedo_mean_device (rt_denoise.hip, the means-form prepare): the live route's running mean with Welford's M2 beside it, and
the two filters on such frames, bit for bit against the numpy restatements of tests/live_denoise_helpers.py.

The reduction's expected frames come from the CPU oracle's single-sample renders (live_helpers.oracle_samples), folded by the
restatement; frames are 20 x 12, so every tile of the bottom row and the last column has padding pixels, and 5 samples.  The filters
run on synthetic (m, M2, n) frames of 1 x 1, 5 x 3, 33 x 9 and 70 x 40 — across the 32 x 8 tile in both directions and across the
stride-2 halo — with K = 1..5 (both LDS kernels and the global one), with NaN, +-inf and negative M2 entries.

Agreement with the sums form (a tolerance, the one test here that is not bit equality): on random_spheres_20x12's five oracle samples
the two numpy restatements, M2 / (n - 1) and (Q - S * m) / (n - 1), differ by at most 2.729e-10 relative over the 558 of 720 values
where both variances are positive (rel = |a - b| / max(a, b); the sums form is negative in 2 of the others); the device is held to
10 x the figure the test computes from those same samples.

Quality (Cornell box 64 x 64, 16 samples through the live route, against the library's own 1024-spp mean under another seed): the test
prints both mean squared errors before it asserts that the filtered frame's is the smaller (DESIGN.md section 5 "Live denoise")."""
import numpy as np
import pytest

import live_denoise_helpers as ldh
from adaptive_helpers import SENTINEL, assert_bits

pytestmark = pytest.mark.gpu

SEED = 9
N = 5
# name -> (scene, width, aspect, (w, h)): the aspect sits half a row above w / h so that the height's truncation is safe
CASES = {
    "random_spheres_20x12": (0, 20, 20 / 12.5, (20, 12)),
    "cornell_20x12": (6, 20, 20 / 12.5, (20, 12)),
    "cornell_smoke_20x12": (7, 20, 20 / 12.5, (20, 12)),  # media draw inside the traversal
}
SPHERES, CORNELL, SMOKE = CASES
_cache, _frames = {}, {}


def expected(rt, oracle, case):
    """(host scene, per-sample colours, [(m, M2) after k samples for k = 0 .. N]), computed once per case and read-only"""
    if case not in _cache:
        scene, width, aspect, size = CASES[case]
        hs = rt.HostScene(scene, width=width, aspect=aspect, spp=N, depth=8)
        assert (hs.width, hs.height) == size and hs.width % 8 and hs.height % 8
        colours = ldh.live_helpers.oracle_samples(rt, oracle, hs, N, SEED)
        states = [(np.zeros(hs.width * hs.height * 3), np.zeros(hs.width * hs.height * 3))]
        for s, c in enumerate(colours):
            states.append(ldh.fold_moments([c], mean=states[-1][0], m2=states[-1][1], first=s))
        m, q = ldh.fold_moments(colours)
        assert_bits(states[N][0], m, "fold: sample by sample against all at once: mean")
        assert_bits(states[N][1], q, "fold: sample by sample against all at once: M2")
        assert_bits(m, ldh.live_helpers.fold(colours), "the restatement's mean against the live route's")
        assert (q > 0.0).sum() >= 48 and (q >= 0.0).all(), f"{case}: M2 is zero nearly everywhere: choose another scene"
        for pair in states:
            for a in pair:
                a.setflags(write=False)
        _cache[case] = (hs, colours, states)
    return _cache[case]


def render_on_device(rt, ds, hs, ranges, fill=SENTINEL, rgba=True, guard=64, state_in=None):
    """rt_render_mean_moments_device over each range in turn into two torch buffers pre-filled with `fill` (or holding state_in); the
    display buffer sits between two guards of 0xA5 bytes, the two frames between guards of 8 doubles.  Returns (mean, m2, rgba8 (h, w, 4)
    or None, launches per call)."""
    import torch
    n_pix = hs.width * hs.height
    stream = torch.cuda.current_stream().cuda_stream
    bufs = []
    for k in range(2):
        d = torch.full((8 + n_pix * 3 + 8,), int(fill), dtype=torch.int64, device="cuda").view(torch.float64)
        if state_in is not None:
            d[8:-8] = torch.from_numpy(np.ascontiguousarray(state_in[k], dtype=np.float64).reshape(-1)).cuda()
        bufs.append(d)
    b = torch.full((guard + n_pix * 4 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    launches = []
    for begin, end in ranges:
        ds.render_mean_moments_device(rt.render_params(seed=SEED, sample_begin=begin, sample_end=end), bufs[0].data_ptr() + 64,
                                      bufs[1].data_ptr() + 64, b.data_ptr() + guard if rgba else 0, stream)
        launches.append(rt.debug_last_launch()["launches"])
    torch.cuda.synchronize()
    raw = b.cpu().numpy()
    out = [d.cpu().numpy() for d in bufs]
    for o in out:
        assert (o[:8].view(np.int64) == int(fill)).all() and (o[-8:].view(np.int64) == int(fill)).all(), "values outside a frame were written"
    assert (raw[:guard] == 0xA5).all() and (raw[guard + n_pix * 4:] == 0xA5).all(), "bytes outside the display frame were written"
    if not rgba:
        assert (raw == 0xA5).all(), "a display frame nobody asked for was written"
    frame = raw[guard:guard + n_pix * 4].reshape(hs.height, hs.width, 4)
    return out[0][8:-8], out[1][8:-8], (frame if rgba else None), launches


def mean_route(rt, ds, hs, n):
    """(mean, rgba8) of rt_render_mean_device over [0, n)"""
    import torch
    n_pix = hs.width * hs.height
    d = torch.zeros(n_pix * 3, dtype=torch.float64, device="cuda")
    b = torch.zeros(n_pix * 4, dtype=torch.uint8, device="cuda")
    ds.render_mean_device(rt.render_params(seed=SEED, sample_end=n), d.data_ptr(), b.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d.cpu().numpy(), b.cpu().numpy().reshape(hs.height, hs.width, 4)


@pytest.mark.parametrize("case", list(CASES))
def test_mean_and_m2_equal_the_fold_of_the_oracles_samples(rt, oracle, gpu, case):
    hs, colours, states = expected(rt, oracle, case)
    ds = rt.DeviceScene(hs)
    mean, m2, frame, launches = render_on_device(rt, ds, hs, [(0, N)])
    assert launches == [1]
    assert_bits(mean, states[N][0], f"{case}: d_mean against the fold")
    assert_bits(m2, states[N][1], f"{case}: d_m2 against the fold")
    plain, plain_frame = mean_route(rt, ds, hs, N)
    assert_bits(mean, plain, f"{case}: d_mean against rt_render_mean_device")
    assert np.array_equal(frame, plain_frame), f"{case}: display bytes against rt_render_mean_device's"
    assert np.array_equal(frame, ldh.display(rt, states[N][0].reshape(hs.height, hs.width, 3))), f"{case}: display bytes"
    assert len(np.unique(frame[:, :, :3])) > 8, "a frame of next to one colour shows nothing"
    # continuation at a split point; a call that starts at sample 0 does not read either buffer, whatever NaN it holds
    for a in (1, 3):
        mean, m2, frame, _ = render_on_device(rt, ds, hs, [(0, a), (a, N)])
        assert_bits(mean, states[N][0], f"{case}: [0, {a}) then [{a}, {N}): mean")
        assert_bits(m2, states[N][1], f"{case}: [0, {a}) then [{a}, {N}): M2")
        assert np.array_equal(frame, plain_frame)
    part = render_on_device(rt, ds, hs, [(0, 3)], fill=np.uint64(0xFFFFFFFFFFFFFFFF).view(np.int64), rgba=False)
    assert_bits(part[0], states[3][0], f"{case}: [0, 3) into NaN: mean")
    assert_bits(part[1], states[3][1], f"{case}: [0, 3) into NaN: M2")
    # ... and a call that does not start there reads both: from a state the caller made up, the recurrence goes on from it
    made_up = (np.linspace(0.0, 1.0, mean.size), np.linspace(2.0, 0.5, mean.size))
    mean, m2, _, _ = render_on_device(rt, ds, hs, [(3, N)], state_in=made_up, rgba=False)
    want = ldh.fold_moments(colours[3:], mean=made_up[0], m2=made_up[1], first=3)
    assert_bits(mean, want[0], f"{case}: [3, {N}) from a caller's state: mean")
    assert_bits(m2, want[1], f"{case}: [3, {N}) from a caller's state: M2")


@pytest.mark.parametrize("case", [SPHERES, CORNELL])
def test_a_call_of_several_launches_gives_one_launchs_bits(rt, oracle, gpu, case):
    """a sample buffer of three sample rows, as tests/test_gpu_live.py forces it: [0, 5) does not fit, and each of the two pipelined
    scratch sets holds one sample: every launch continues both frames with its own absolute divisors; only the last writes the bytes"""
    hs, colours, states = expected(rt, oracle, case)
    row = ((hs.width + 7) // 8) * ((hs.height + 7) // 8) * 64 * 24
    ds = rt.DeviceScene(hs, sample_buffer_bytes=3 * row)
    mean, m2, frame, launches = render_on_device(rt, ds, hs, [(0, N)])
    assert launches[0] >= 3, launches
    assert_bits(mean, states[N][0], f"{case}: [0, {N}) in {launches[0]} launches: mean")
    assert_bits(m2, states[N][1], f"{case}: [0, {N}) in {launches[0]} launches: M2")
    assert np.array_equal(frame, ldh.display(rt, states[N][0].reshape(hs.height, hs.width, 3)))
    mean, m2, frame, launches = render_on_device(rt, ds, hs, [(0, 1), (1, N)])
    assert launches[1] >= 3, launches
    assert_bits(mean, states[N][0], f"{case}: a continuation in {launches[1]} launches: mean")
    assert_bits(m2, states[N][1], f"{case}: a continuation in {launches[1]} launches: M2")
    assert np.array_equal(frame, ldh.display(rt, states[N][0].reshape(hs.height, hs.width, 3)))


@pytest.mark.parametrize("case", [SPHERES, SMOKE])
def test_the_host_buffer_form_gives_the_device_forms_bits(rt, oracle, gpu, case):
    hs, colours, states = expected(rt, oracle, case)
    ds = rt.DeviceScene(hs)
    mean, m2, frame = ds.render_mean_moments(rt.render_params(seed=SEED, sample_end=N), rgba8=True)
    assert mean.shape == m2.shape == (hs.height, hs.width, 3) and frame.shape == (hs.height, hs.width, 4) and frame.dtype == np.uint8
    assert_bits(mean.reshape(-1), states[N][0], f"{case}: rt_render_mean_moments: mean")
    assert_bits(m2.reshape(-1), states[N][1], f"{case}: rt_render_mean_moments: M2")
    assert np.array_equal(frame, ldh.display(rt, mean))
    a, b = ds.render_mean_moments(rt.render_params(seed=SEED, sample_end=2))
    assert_bits(a.reshape(-1), states[2][0], f"{case}: [0, 2): mean")
    assert_bits(b.reshape(-1), states[2][1], f"{case}: [0, 2): M2")
    a2, b2 = ds.render_mean_moments(rt.render_params(seed=SEED, sample_begin=2, sample_end=N), mean=a, m2=b)   # both are uploaded first
    assert a2 is a and b2 is b
    assert_bits(a.reshape(-1), states[N][0], f"{case}: [0, 2) then [2, {N}): mean")
    assert_bits(b.reshape(-1), states[N][1], f"{case}: [0, 2) then [2, {N}): M2")
    nan = np.full((hs.height, hs.width, 3), np.nan)
    c, d = ds.render_mean_moments(rt.render_params(seed=SEED, sample_end=N), mean=nan, m2=nan.copy())
    assert_bits(c.reshape(-1), states[N][0], f"{case}: into NaN: mean")
    assert_bits(d.reshape(-1), states[N][1], f"{case}: into NaN: M2")
    # the scene handle and its scratch, used for this first, still render what they rendered
    assert_bits(ds.render_mean(rt.render_params(seed=SEED, sample_end=N)).reshape(-1), states[N][0], f"{case}: rt_render_mean afterwards")


# ---- the filters on synthetic (m, M2, n) frames ----
SIZES = [(1, 1), (5, 3), (33, 9), (70, 40)]


def frames(w, h):
    if (w, h) not in _frames:
        M, M2, n = ldh.synthetic_means(w, h, 1000 * w + h)
        A = ldh.synthetic_albedo_mean(w, h, 77 * w + h)
        if w * h >= 15:
            assert not np.isfinite(M).all() and not np.isfinite(M2).all() and not np.isfinite(A).all()
            assert (M2 < 0.0).any() and (A[np.isfinite(A)] < 1e-3).any() and (A[np.isfinite(A)] > 1.0).any()
        for a in (M, M2, A):
            a.setflags(write=False)
        _frames[(w, h)] = (M, M2, n, A)
    return _frames[(w, h)]


def filter_on_device(rt, M, M2, n, A=None, guard=64, **kw):
    """rt_denoise_mean_device (A: rt_denoise_albedo_mean_device) into buffers with guards: (means (h, w, 3), bytes (h, w, 4)); nothing
    outside them may be written, and the inputs are inputs"""
    import torch
    h, w = M.shape[:2]
    n_pix = w * h
    d_in = [torch.from_numpy(np.array(a)).cuda() for a in ((M, M2) if A is None else (M, M2, A))]  # (copies: the shared frames are read-only)
    fill = float(np.uint64(0x7FF8DEADBEEF0001).view(np.float64))
    d_out = torch.full((8 + 3 * n_pix + 8,), fill, dtype=torch.float64, device="cuda")
    d_b = torch.full((guard + 4 * n_pix + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ws_bytes = rt.denoise_workspace_bytes(w, h) if A is None else rt.denoise_albedo_workspace_bytes(w, h)
    d_ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if A is None:
        rt.denoise_mean_device(w, h, d_in[0].data_ptr(), d_in[1].data_ptr(), n, d_out.data_ptr() + 64, d_ws.data_ptr(),
                               d_rgba8_ptr=d_b.data_ptr() + guard, params=rt.denoise_params(**kw), stream=stream)
    else:
        rt.denoise_albedo_mean_device(w, h, d_in[0].data_ptr(), d_in[1].data_ptr(), n, d_in[2].data_ptr(), d_out.data_ptr() + 64, d_ws.data_ptr(),
                                      d_rgba8_ptr=d_b.data_ptr() + guard, params=rt.denoise_albedo_params(**kw), stream=stream)
    torch.cuda.synchronize()
    out, raw, ws = d_out.cpu().numpy(), d_b.cpu().numpy(), d_ws.cpu().numpy()
    assert np.isnan(out[:8]).all() and np.isnan(out[-8:]).all(), "values outside d_mean_out were written"
    assert (raw[:guard] == 0xA5).all() and (raw[guard + 4 * n_pix:] == 0xA5).all(), "bytes outside d_rgba8 were written"
    assert (ws[ws_bytes:] == 0xA5).all(), "bytes behind the workspace were written"
    for got, want, name in zip(d_in, (M, M2, A), ("d_mean", "d_m2", "d_albedo_mean")):
        assert_bits(got.cpu().numpy(), want, f"{name} after the call")
    return out[8:-8].reshape(h, w, 3), raw[guard:guard + 4 * n_pix].reshape(h, w, 4)


@pytest.mark.parametrize("k", range(1, 6))
@pytest.mark.parametrize("w, h", SIZES)
def test_the_means_form_filter_equals_the_definition_bit_for_bit(rt, gpu, w, h, k):
    M, M2, n, _ = frames(w, h)
    want = ldh.denoise_mean(M, M2, n, iterations=k)
    got, rgba = filter_on_device(rt, M, M2, n, iterations=k)
    assert_bits(got, want, f"{w}x{h}, K = {k}")
    assert np.array_equal(rgba, ldh.display(rt, want)), f"{w}x{h}, K = {k}: display bytes"
    if w * h >= 15:
        C0, V0, valid = ldh.prepare_mean(M, M2, n)
        assert valid.any() and not valid.all()
        assert np.isfinite(got[valid]).all(), "a valid pixel took a tap that is not valid"
        assert (got != C0)[valid].any(), "the filter changed nothing"
        assert (V0[(M2 < 0.0).all(axis=2) & valid] == 0.0).all() and ((M2 < 0.0).all(axis=2) & valid).any()
    # one sample: no pixel is valid, the output is the input mean — its NaN and inf entries as they are — and so are its bytes
    one, one_rgba = filter_on_device(rt, M, M2, 1, iterations=k)
    assert_bits(one, M, f"{w}x{h}, K = {k}, samples = 1")
    assert np.array_equal(one_rgba, ldh.display(rt, M))


def test_other_parameters_are_honoured_and_the_blocking_wrapper_is_the_same_call(rt, gpu):
    w, h = 70, 40
    M, M2, n, A = frames(w, h)
    base, _ = filter_on_device(rt, M, M2, n)
    for kw in (dict(sigma=1.0), dict(sigma=16.0, iterations=3), dict(eps=1e-2, iterations=2)):
        got, rgba = filter_on_device(rt, M, M2, n, **kw)
        want = ldh.denoise_mean(M, M2, n, **{**ldh.DEFAULTS, **kw})
        assert_bits(got, want, str(kw))
        assert np.array_equal(rgba, ldh.display(rt, want))
        assert not np.array_equal(got, base, equal_nan=True), f"{kw} changed nothing"
    # another sample count over the same frames is another filter: n enters V0 twice
    assert_bits(filter_on_device(rt, M, M2, 3)[0], ldh.denoise_mean(M, M2, 3), "samples = 3")
    assert not np.array_equal(filter_on_device(rt, M, M2, 3)[0], base, equal_nan=True)
    mean, rgba = rt.denoise_mean(M, M2, n, rgba8=True)
    assert_bits(mean, base, "rt.denoise_mean against rt.denoise_mean_device")
    assert rgba.shape == (h, w, 4) and np.array_equal(rgba, ldh.display(rt, base))
    assert_bits(rt.denoise_mean(M, M2, n, iterations=2, sigma=2.0), ldh.denoise_mean(M, M2, n, iterations=2, sigma=2.0), "rt.denoise_mean(**kw)")
    guided = rt.denoise_albedo_mean(M, M2, n, A, iterations=2, sigma_albedo=0.2)
    assert_bits(guided, ldh.denoise_albedo_mean(M, M2, n, A, iterations=2, sigma_albedo=0.2), "rt.denoise_albedo_mean(**kw)")


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("w, h", SIZES)
def test_the_guided_means_form_equals_its_definition_and_the_plain_one_at_albedo_one(rt, gpu, w, h, k):
    M, M2, n, A = frames(w, h)
    want = ldh.denoise_albedo_mean(M, M2, n, A, iterations=k)
    got, rgba = filter_on_device(rt, M, M2, n, A, iterations=k)
    assert_bits(got, want, f"{w}x{h}, K = {k}")
    assert np.array_equal(rgba, ldh.display(rt, want)), f"{w}x{h}, K = {k}: display bytes"
    if w * h >= 15:
        C0, V0, valid, a, d = ldh.prepare_albedo_mean(M, M2, n, A, ldh.ALBEDO_DEFAULTS["albedo_floor"])
        assert valid.any() and not valid.all() and (d[valid] == 1e-3).any() and (w * h < 100 or (d[valid] > 1.0).any()), "the synthetic albedo misses the floor"
        assert np.isfinite(got[valid]).all()
        plain = ldh.denoise_mean(M, M2, n, iterations=k)
        assert not np.array_equal(got, plain, equal_nan=True), "the guide changed nothing"
    ones = np.ones_like(M)
    same, same_rgba = filter_on_device(rt, M, M2, n, ones, iterations=k)
    plain, plain_rgba = filter_on_device(rt, M, M2, n, iterations=k)
    assert_bits(same, plain, f"{w}x{h}, K = {k}: albedo mean 1 everywhere against the plain means form")
    assert np.array_equal(same_rgba, plain_rgba)
    one, _ = filter_on_device(rt, M, M2, 1, A, iterations=k)
    assert_bits(one, M, f"{w}x{h}, K = {k}, samples = 1")
    if k == 2:
        kw = dict(iterations=2, sigma=2.0, eps=1e-3, sigma_albedo=0.1, albedo_floor=0.05)
        assert_bits(filter_on_device(rt, M, M2, n, A, **kw)[0], ldh.denoise_albedo_mean(M, M2, n, A, **kw), f"{w}x{h}: {kw}")


def test_the_variance_agrees_with_the_sums_forms_on_one_rendered_scene(rt, oracle, gpu):
    """M2 / (n - 1) of this route against (Q - S * m) / (n - 1) of rt_render_moments under the same seed, over the values where both are
    positive, rel = |a - b| / max(a, b).  The bound is 10 x what the two numpy restatements show on the oracle's samples of the same
    case (random_spheres_20x12, 5 samples: 2.729e-10, where a sky pixel's samples are nearly equal and Q - S * m cancels; the two
    Cornell cases, whose lit pixels' samples differ by much of their size, show 3.0e-16 and 4.3e-16).  The device equals the
    restatements bit for bit, so the margin is slack; the bound is there to catch a wrong formula."""
    hs, colours, states = expected(rt, oracle, SPHERES)
    n = float(N)
    v_sums, S, Q = ldh.sums_variance(colours)
    v_means = states[N][1] / (n - 1.0)

    def rel(a, b):
        both = (a > 0.0) & (b > 0.0)
        assert both.sum() > a.size // 2, int(both.sum())
        return float((np.abs(a - b)[both] / np.maximum(a, b)[both]).max())

    bound = 10.0 * rel(v_means, v_sums)
    ds = rt.DeviceScene(hs)
    p = rt.render_params(seed=SEED, sample_end=N)
    mean, m2 = ds.render_mean_moments(p)
    s, q = ds.render_moments(p)
    got_means = m2.reshape(-1) / (n - 1.0)
    got_sums = ((q - s * (s / n)) / (n - 1.0)).reshape(-1)
    figure = rel(got_means, got_sums)
    print(f"largest relative difference of the two variances: restatements {bound / 10.0:.3e}, device {figure:.3e}, bound {bound:.3e}")
    assert 0.0 < bound < 1e-8, bound
    assert figure <= bound, (figure, bound)
    assert np.allclose(mean.reshape(-1), s.reshape(-1) / n, rtol=1e-14, atol=0.0)


def test_end_to_end_the_live_routes_filtered_frame_is_closer_to_the_converged_one(rt, gpu):
    """Cornell box 64 x 64, 16 samples in passes of one through rt_render_mean_moments_device, the filter after every pass into a
    separate frame: the running frames are never the filter's output, and the last filtered frame beats the unfiltered mean"""
    import torch
    hs = rt.HostScene(6, width=64, aspect=1.0, spp=16, depth=8)
    w, h = hs.width, hs.height
    assert (w, h) == (64, 64)
    ds = rt.DeviceScene(hs)
    stream = torch.cuda.current_stream().cuda_stream
    d_mean, d_m2, d_shown = (torch.full((3 * w * h,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
    d_b = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
    d_ws = torch.empty(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    for s in range(16):
        ds.render_mean_moments_device(rt.render_params(seed=5, sample_begin=s, sample_end=s + 1), d_mean.data_ptr(), d_m2.data_ptr(), 0, stream)
        rt.denoise_mean_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), s + 1, d_shown.data_ptr(), d_ws.data_ptr(), d_rgba8_ptr=d_b.data_ptr(),
                               stream=stream)
        if s == 0:
            torch.cuda.synchronize()
            assert torch.equal(d_shown.view(torch.int64), d_mean.view(torch.int64)), "one sample: the frame shown is the mean"
    torch.cuda.synchronize()
    mean, m2, shown = (d.cpu().numpy().reshape(h, w, 3) for d in (d_mean, d_m2, d_shown))
    rgba = d_b.cpu().numpy().reshape(h, w, 4)
    one_call = ds.render_mean_moments(rt.render_params(seed=5, sample_end=16))
    assert_bits(mean, one_call[0], "sixteen passes of one sample against one call: mean")
    assert_bits(m2, one_call[1], "sixteen passes of one sample against one call: M2")
    want = ldh.denoise_mean(mean, m2, 16)
    assert_bits(shown, want, "the last filtered frame against numpy on the same mean and M2")
    assert np.array_equal(rgba, ldh.display(rt, want))
    ref = ds.render(rt.render_params(seed=77, sample_end=1024)).reshape(mean.shape) / 1024.0
    mse_noisy, mse_denoised = float(np.mean((mean - ref) ** 2)), float(np.mean((shown - ref) ** 2))
    print(f"MSE against the 1024-spp mean: 16 samples {mse_noisy:.6e}, filtered {mse_denoised:.6e}, ratio {mse_denoised / mse_noisy:.4f}")
    assert mse_denoised < mse_noisy, (mse_denoised, mse_noisy)
