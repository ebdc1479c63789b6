"""rt_render_mean_device / rt_render_mean / rt_resolve_rgba8_device (rt_kernel.hip mean_samples_kernel, resolve_rgba8_kernel): the
running-mean frame of the reference's live_render and its RGBA8 display bytes.

The expected frame is always built from the CPU oracle: sample s's colour is orc_render over [s, s + 1) (0 + c), folded with
m = m + (c - m) / (s + 1) in numpy (live_helpers.fold: elementwise f64, no contraction, a true division).  Before the GPU is looked
at, every expected frame must differ in bits from S / n and from S * (1 / n), S the oracle's sum: a library that divides a sum cannot
pass.  Frames are tiny and neither side is a multiple of 8, so edge tiles with padding pixels exist.  An oracle frame is computed once
per case and shared."""

import numpy as np
import pytest

import live_helpers
from adaptive_helpers import SENTINEL, assert_bits, bits

pytestmark = pytest.mark.gpu

SEED = 9
# name -> (scene, width, aspect, (w, h), samples): the aspect sits half a row above w / h so that the height's truncation is safe
CASES = {
    "random_spheres_44x27": (0, 44, 44 / 27.5, (44, 27), 7),
    "cornell_28x20": (6, 28, 28 / 20.5, (28, 20), 7),
    "cornell_smoke_20x12": (7, 20, 20 / 12.5, (20, 12), 4),  # media draw inside the traversal
}
SPHERES, CORNELL, SMOKE = CASES
WALKS = ("own trees, two children", "own trees, four children", "reference order")

_cache = {}


def walk_options(rt, walk):
    return {"own trees, two children": dict(walk=rt.RT_WALK_OWN_TREES, wide=0), "own trees, four children": dict(walk=rt.RT_WALK_OWN_TREES, wide=1),
            "reference order": dict(walk=rt.RT_WALK_REFERENCE_ORDER)}[walk]


def expected(rt, oracle, case):
    """(host scene, per-sample colours, means[k] after k samples, the oracle's sum over all n); the precondition is asserted here, on
    the expected frame alone"""
    if case not in _cache:
        scene, width, aspect, size, n = CASES[case]
        hs = rt.HostScene(scene, width=width, aspect=aspect, spp=n, depth=8)
        assert (hs.width, hs.height) == size and hs.width % 8 and hs.height % 8
        colours = live_helpers.oracle_samples(rt, oracle, hs, n, SEED)
        means = [np.zeros(hs.width * hs.height * 3)]
        for s, c in enumerate(colours):
            means.append(live_helpers.fold([c], mean=means[-1], first=s))
        assert_bits(means[n], live_helpers.fold(colours), "fold: sample by sample against all at once")
        total = oracle.render(hs, rt.render_params(seed=SEED, sample_end=n))
        want = means[n]
        assert (bits(want) != bits(total / float(n))).any(), f"{case}: the running mean equals S / n in every value: choose another scene"
        assert (bits(want) != bits(total * (1.0 / float(n)))).any(), f"{case}: the running mean equals S * (1 / n) in every value: choose another scene"
        for m in means:
            m.setflags(write=False)
        total.setflags(write=False)
        _cache[case] = (hs, colours, means, total)
    return _cache[case]


def render_mean_on_device(rt, ds, hs, ranges, fill=SENTINEL, rgba=True, guard=64, mean_in=None):
    """rt_render_mean_device over each range in turn into one torch buffer pre-filled with `fill` (or holding mean_in); the display
    buffer sits between two guards of 0xA5 bytes.  Returns (mean, rgba8 (h, w, 4) or None, the guards' bytes, launches per call)."""
    import torch
    n_pix = hs.width * hs.height
    stream = torch.cuda.current_stream().cuda_stream
    if mean_in is None:
        d = torch.full((n_pix * 3,), int(fill), dtype=torch.int64, device="cuda").view(torch.float64)
    else:
        d = torch.from_numpy(np.ascontiguousarray(mean_in, dtype=np.float64).reshape(-1)).cuda()
    b = torch.full((guard + n_pix * 4 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    launches = []
    for begin, end in ranges:
        ds.render_mean_device(rt.render_params(seed=SEED, sample_begin=begin, sample_end=end), d.data_ptr(),
                              b.data_ptr() + guard if rgba else 0, stream)
        launches.append(rt.debug_last_launch()["launches"])
    torch.cuda.synchronize()
    raw = b.cpu().numpy()
    frame = raw[guard:guard + n_pix * 4].reshape(hs.height, hs.width, 4)
    return d.cpu().numpy(), (frame if rgba else None), np.concatenate([raw[:guard], raw[guard + n_pix * 4:]]), launches


def check_display(rt, hs, frame, mean, what):
    """the display bytes of `mean`: RGB = color_to_rgb(mean) as the host library computes it at spp 1, alpha 255"""
    assert frame.shape == (hs.height, hs.width, 4)
    assert np.array_equal(frame[:, :, :3], rt.resolve_rgb8_host(hs.width, hs.height, 1, mean)), f"{what}: RGB bytes"
    assert (frame[:, :, 3] == 255).all(), f"{what}: alpha"


@pytest.mark.parametrize("case, walk", [(c, w) for c in (SPHERES, CORNELL) for w in WALKS] + [(SMOKE, "default")])
def test_the_mean_equals_the_recurrence_over_the_oracles_samples(rt, oracle, gpu, case, walk):
    hs, colours, means, total = expected(rt, oracle, case)
    n = len(colours)
    ds = rt.DeviceScene(hs, **(walk_options(rt, walk) if walk != "default" else {}))
    got, frame, guards, launches = render_mean_on_device(rt, ds, hs, [(0, n)])
    assert_bits(got, means[n], f"{case}, {walk}: [0, {n})")
    assert launches == [1]
    # display bytes: the fused frame is the stand-alone resolve's, the host library's RGB with alpha 255, and nothing beyond it
    check_display(rt, hs, frame, means[n], f"{case}, {walk}")
    assert (guards == 0xA5).all(), "bytes outside the display frame were written"
    import torch
    d = torch.from_numpy(np.array(means[n])).cuda()
    b = torch.full((64 + hs.width * hs.height * 4 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rt.resolve_rgba8_device(hs.width, hs.height, d.data_ptr(), b.data_ptr() + 64, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    alone = b.cpu().numpy()
    assert np.array_equal(alone[64:-64].reshape(frame.shape), frame), "rt_resolve_rgba8_device differs from the fused frame"
    assert (alone[:64] == 0xA5).all() and (alone[-64:] == 0xA5).all(), "rt_resolve_rgba8_device wrote outside its frame"
    assert len(np.unique(frame[:, :, :3])) > 8, "a frame of next to one colour shows nothing"


@pytest.mark.parametrize("case", [SPHERES, CORNELL])
def test_a_call_continues_the_mean_and_sample_zero_ignores_the_buffer(rt, oracle, gpu, case):
    hs, colours, means, total = expected(rt, oracle, case)
    ds = rt.DeviceScene(hs)
    got, frame, _, _ = render_mean_on_device(rt, ds, hs, [(0, 3), (3, 7)])
    assert_bits(got, means[7], f"{case}: [0, 3) then [3, 7)")
    check_display(rt, hs, frame, means[7], f"{case}: the second call's frame")
    part, frame3, _, _ = render_mean_on_device(rt, ds, hs, [(0, 3)])
    assert_bits(part, means[3], f"{case}: [0, 3)")
    check_display(rt, hs, frame3, means[3], f"{case}: [0, 3)")
    # a buffer of NaN (the sentinel is one; so is the all-ones pattern) is not read by a call that starts at sample 0 ...
    for fill in (SENTINEL, np.uint64(0xFFFFFFFFFFFFFFFF).view(np.int64)):
        got, _, _, _ = render_mean_on_device(rt, ds, hs, [(0, 7)], fill=fill, rgba=False)
        assert_bits(got, means[7], f"{case}: [0, 7) into a buffer of NaN")
    # ... and IS read by one that does not: from a mean the caller made up, the recurrence goes on from there
    made_up = np.linspace(0.0, 1.0, hs.width * hs.height * 3)
    got, _, _, _ = render_mean_on_device(rt, ds, hs, [(3, 7)], mean_in=made_up, rgba=False)
    assert_bits(got, live_helpers.fold(colours[3:7], mean=made_up, first=3), f"{case}: [3, 7) from a caller's mean")


@pytest.mark.parametrize("case", [SPHERES, CORNELL])
def test_a_call_of_several_launches_gives_one_launchs_bits(rt, oracle, gpu, case):
    """a sample buffer of three sample rows: [0, 7) does not fit; each of the two pipelined scratch sets holds one sample (without
    pipelining the one set holds three): seven launches (three), each continuing the frame with its own absolute divisors; only the
    last writes the display frame"""
    hs, colours, means, total = expected(rt, oracle, case)
    row = ((hs.width + 7) // 8) * ((hs.height + 7) // 8) * 64 * 24
    ds = rt.DeviceScene(hs, sample_buffer_bytes=3 * row)
    got, frame, guards, launches = render_mean_on_device(rt, ds, hs, [(0, 7)])
    assert launches[0] >= 3, launches
    assert_bits(got, means[7], f"{case}: [0, 7) in {launches[0]} launches")
    check_display(rt, hs, frame, means[7], f"{case}: several launches")
    assert (guards == 0xA5).all()
    assert not np.array_equal(frame[:, :, :3], rt.resolve_rgb8_host(hs.width, hs.height, 1, means[6])), "means[6] and means[7] show the same frame"
    # a continuation that is itself several launches
    got, frame, _, launches = render_mean_on_device(rt, ds, hs, [(0, 2), (2, 7)])
    assert launches[1] >= 3, launches
    assert_bits(got, means[7], f"{case}: [0, 2) then [2, 7) in {launches[1]} launches")
    check_display(rt, hs, frame, means[7], f"{case}: continuation in several launches")


@pytest.mark.parametrize("case", [SPHERES, SMOKE])
def test_the_host_buffer_form_gives_the_device_forms_bits(rt, oracle, gpu, case):
    hs, colours, means, total = expected(rt, oracle, case)
    n = len(colours)
    ds = rt.DeviceScene(hs)
    mean, frame = ds.render_mean(rt.render_params(seed=SEED, sample_end=n), rgba8=True)
    assert mean.shape == (hs.height, hs.width, 3) and frame.shape == (hs.height, hs.width, 4) and frame.dtype == np.uint8
    assert_bits(mean.reshape(-1), means[n], f"{case}: rt_render_mean [0, {n})")
    check_display(rt, hs, frame, means[n], f"{case}: rt_render_mean")
    # continuation: the caller's mean is uploaded first
    part = ds.render_mean(rt.render_params(seed=SEED, sample_end=2))
    assert_bits(part.reshape(-1), means[2], f"{case}: rt_render_mean [0, 2)")
    both = ds.render_mean(rt.render_params(seed=SEED, sample_begin=2, sample_end=n), mean=part)
    assert both is part
    assert_bits(both.reshape(-1), means[n], f"{case}: rt_render_mean [0, 2) then [2, {n})")
    # sample 0 does not read the host buffer either; no display frame asked for, none written
    nan = np.full((hs.height, hs.width, 3), np.nan)
    assert_bits(ds.render_mean(rt.render_params(seed=SEED, sample_end=n), mean=nan).reshape(-1), means[n], f"{case}: rt_render_mean into NaN")
    with pytest.raises(rt.RtError, match="sample_begin"):
        ds.render_mean(rt.render_params(seed=SEED, sample_begin=2, sample_end=n))


@pytest.mark.parametrize("case", list(CASES))
def test_rt_render_still_equals_the_oracles_sum(rt, oracle, gpu, case):
    hs, colours, means, total = expected(rt, oracle, case)
    ds = rt.DeviceScene(hs)
    ds.render_mean(rt.render_params(seed=SEED, sample_end=len(colours)))  # (the same scene handle and scratch, used for a mean first)
    assert_bits(ds.render(rt.render_params(seed=SEED, sample_end=len(colours))), total, f"{case}: rt_render after rt_render_mean")
