"""Robust frames on the device (rt_robust_device) against the host mirror and the numpy restatement of include/rt_amd.h "robust frames"
(tests/robust_helpers.py), bit for bit: every mode at K on both sides of every boundary between the kernel's forms, sums and means, every
form through the debug hook, with and without M2, a second call into used outputs, the route over a real render, identical copies, and
the robust (mean, M2) through the means-form filter."""
import numpy as np
import pytest

import live_denoise_helpers as ldh
import robust_helpers as rh

pytestmark = pytest.mark.gpu

MODE_KW = [dict(mode="mean"), dict(mode="trim", trim=2), dict(mode="median"), dict(mode="gini"), dict(mode="gini", gain=2.5)]


@pytest.fixture(scope="module")
def stacks():
    """per (K, w, h): the stack — made once, never written"""
    out = {}
    for K in rh.KS:
        for w, h in rh.GPU_SHAPES:
            s = rh.stack(K, w, h, seed=w)
            s.setflags(write=False)
            out[(K, w, h)] = s
    return out


@pytest.fixture(scope="module")
def restated(stacks):
    """the restatement's (out, M2) of a stack of `stacks` at 7 samples per block, computed once per (stack, params)"""
    cache = {}

    def get(key, **kw):
        k = (key, tuple(sorted(kw.items())))
        if k not in cache:
            cache[k] = rh.robust(stacks[key], 7, **kw)
        return cache[k]
    return get


@pytest.fixture()
def form(rt):
    """sets the kernel form, and puts the built-in rule back afterwards"""
    lib = rt.amd_lib()
    yield lambda slots: lib.rt_debug_set_robust_form(slots)
    lib.rt_debug_set_robust_form(0)


@pytest.mark.parametrize("K", rh.KS)
def test_device_bits_are_the_mirrors_and_the_restatements(rt, gpu, stacks, K):
    for w, h in rh.GPU_SHAPES:
        s = stacks[(K, w, h)]
        for spp in (7, 1):
            for kw in MODE_KW:
                want, want_m2 = rh.robust(s, spp, **kw)
                got, got_m2 = rt.robust(s, spp, m2=True, **kw)
                assert rh.same_bits(got, want), (w, h, spp, kw, rh.differing(got, want))
                assert rh.same_bits(got_m2, want_m2), (w, h, spp, kw, rh.differing(got_m2, want_m2))
        host, host_m2 = rt.robust_host(s, 7, m2=True)
        got, got_m2 = rt.robust(s, 7, m2=True)
        assert rh.same_bits(got, host) and rh.same_bits(got_m2, host_m2), (w, h)
        # without d_m2_out the means are the same
        assert rh.same_bits(rt.robust(s, 7), got), (w, h)


@pytest.mark.parametrize("slots", [4, 8, 16, 32])
def test_every_kernel_form_gives_the_same_bits(rt, gpu, stacks, restated, form, slots):
    """A form runs every K it has the slots for (a smaller one falls back to the smallest that fits), so each form is driven at the K
    just below and at its own size and the next form's first K, with and without M2."""
    assert form(slots) == 0, "the built-in rule must have been in force"
    assert form(slots) == slots
    for K in rh.KS:
        for w, h in ((65, 17), (256, 8)):
            s = stacks[(K, w, h)]
            for kw in (dict(mode="gini"), dict(mode="trim", trim=2)):
                want, want_m2 = restated((K, w, h), **kw)
                got, got_m2 = rt.robust(s, 7, m2=True, **kw)
                assert rh.same_bits(got, want) and rh.same_bits(got_m2, want_m2), (K, w, h, kw)
                assert rh.same_bits(rt.robust(s, 7, **kw), want), (K, w, h, kw)
    assert form(0) == slots and form(5) == 0 and form(0) == 8 and form(1000) == 0 and form(-3) == 32


def test_a_second_call_into_the_same_outputs_gives_the_same_bits(rt, gpu, stacks):
    import torch
    K, w, h = 9, 65, 17
    s = stacks[(K, w, h)]
    want, want_m2 = rh.robust(s, 7)
    stream = torch.cuda.current_stream().cuda_stream
    d_s = torch.from_numpy(np.array(s)).cuda()
    d_other = torch.from_numpy(rh.stack(K, w, h, seed=99, special=False) * 50.0).cuda()
    d_out = torch.full((2, h, w, 3), float("nan"), dtype=torch.float64, device="cuda")
    got = []
    for d_stack in (d_s, d_other, d_s):
        rt.robust_device(w, h, K, d_stack.data_ptr(), 7, d_out[0].data_ptr(), d_m2_out_ptr=d_out[1].data_ptr(), stream=stream)
        torch.cuda.synchronize()
        got.append(d_out.cpu().numpy())
    assert rh.same_bits(got[0][0], want) and rh.same_bits(got[0][1], want_m2)
    assert rh.same_bits(got[2], got[0]) and not rh.same_bits(got[1], got[0])
    assert rh.same_bits(d_s.cpu().numpy(), s), "the call must leave d_stack untouched"


def test_identical_copies_of_a_frame_give_the_frame(rt, gpu):
    frame = np.abs(rh.stack(1, 65, 17, seed=5, special=False)[0])
    for K in (1, 2, 4, 8):
        mean, m2 = rt.robust(np.repeat(frame[None], K, axis=0), 1, m2=True, mode="mean")
        assert rh.same_bits(mean, frame) and rh.same_bits(m2, np.zeros_like(frame)), K
        # and as sums of 2^j samples each: the block means are exact
        assert rh.same_bits(rt.robust(np.repeat(frame[None] * 4.0, K, axis=0), 4, mode="mean"), frame), K


@pytest.fixture(scope="module")
def simple_light(rt):
    hs = rt.HostScene(5, scene_seed=1, width=32, aspect=4.0 / 3.0, spp=16, depth=8)   # simple_light: an emitter of radiance 4
    assert (hs.width, hs.height) == (32, 24)
    return hs, rt.DeviceScene(hs, device=0)


def test_render_robust_composes_render_views_and_the_combiner(rt, gpu, simple_light):
    hs, ds = simple_light
    cam = hs.camera
    views = [(cam, 5 + k) for k in range(4)]
    stack = ds.render_views(rt.render_params(sample_end=4), views)
    assert stack.shape == (4, 24, 32, 3)
    for k in (0, 3):   # a view is render() under its seed
        assert rh.same_bits(stack[k].reshape(-1), ds.render(rt.render_params(seed=5 + k, sample_end=4)))
    for kw in (dict(), dict(mode="median"), dict(mode="trim", trim=1)):
        want, want_m2 = rt.robust_host(stack, 4, m2=True, **kw)
        mean, m2 = ds.render_robust(rt.render_params(seed=5), 4, **kw)
        assert rh.same_bits(mean, want) and rh.same_bits(m2, want_m2), kw
    assert rh.same_bits(ds.render_robust(rt.render_params(seed=5, sample_end=16), 4)[0], rt.robust_host(stack, 4))
    assert np.isfinite(want).all() and want.max() > 1.0 and len(np.unique(want)) > 8
    with pytest.raises(rt.RtError, match="does not divide"):
        ds.render_robust(rt.render_params(seed=5), 3)
    with pytest.raises(rt.RtError, match="blocks"):
        ds.render_robust(rt.render_params(seed=5), 0)


def test_the_robust_frame_goes_into_the_means_form_filter(rt, gpu, simple_light):
    hs, ds = simple_light
    mean, m2 = ds.render_robust(rt.render_params(seed=5), 4)
    got = rt.denoise_mean(mean, m2, 4)
    stack = ds.render_views(rt.render_params(sample_end=4), [(hs.camera, 5 + k) for k in range(4)])
    r_mean, r_m2 = rh.robust(stack, 4)
    want = ldh.denoise_mean(r_mean, r_m2, 4)
    assert rh.same_bits(got, want), rh.differing(got, want)
    assert not rh.same_bits(got, mean), "the filter must have changed the frame"
