"""Frame metrics on the GPU: rt_frame_error_device and rt_frame_noise_device against the host mirror and the numpy restatement of
include/rt_amd.h "frame metrics", bit for bit at the sizes where the reduction tree changes shape; what the calls leave alone (inputs,
workspace bytes beyond the reported size); two streams; a real render; and DeviceScene.render_until's stopping rule."""
import numpy as np
import pytest

import metrics_helpers as mh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    """per size: the frame pair, the moments in both forms and the spp map, made once (the wrappers upload them and never write them)"""
    out = {}
    for w, h in mh.SIZES:
        frame, ref = mh.frame_pair(w, h)
        S, Q = mh.moments(w, h, 8)
        M, M2 = mh.mean_moments(w, h, 8)
        out[(w, h)] = dict(frame=frame, ref=ref, S=S, Q=Q, M=M, M2=M2, map=mh.spp_map_for(w, h))
    return out


def _error_cases(e):
    """(args, kw) of frame_error: sums with a uniform count, sums with an spp map, means"""
    return [((e["frame"], 12, e["ref"], 48), {}), ((e["frame"], 1, e["ref"], 3), dict(spp_map=e["map"])), ((e["frame"], 1, e["ref"], 1), dict(eps=1e-4, peak=4.0))]


def _noise_cases(e):
    return [((e["S"], e["Q"], 8), {}), ((e["S"], e["Q"], 8), dict(spp_map=e["map"])), ((e["M"], e["M2"], 8), dict(form="means", eps=1e-3))]


@pytest.mark.parametrize("w,h", mh.SIZES)
def test_the_device_values_are_the_mirrors_and_the_restatements(rt, gpu, inputs, w, h):
    e = inputs[(w, h)]
    for args, kw in _error_cases(e):
        dev, host, want = rt.frame_error(*args, **kw), rt.frame_error_host(*args, **kw), mh.frame_error(*args, **kw)
        assert mh.same_bits(dev, host, mh.ERROR_FIELDS), (w, h, kw, dev, host)
        assert mh.same_bits(dev, want, mh.ERROR_FIELDS), (w, h, kw, dev, want)
        assert dev["count"] == (w * h - 3 if w * h >= 8 else w * h)
    for args, kw in _noise_cases(e):
        dev, host, want = rt.frame_noise(*args, **kw), rt.frame_noise_host(*args, **kw), mh.frame_noise(*args, **kw)
        assert mh.same_bits(dev, host, mh.NOISE_FIELDS), (w, h, kw, dev, host)
        assert mh.same_bits(dev, want, mh.NOISE_FIELDS), (w, h, kw, dev, want)
        if "spp_map" in kw and w * h >= 8:
            assert 0 < dev["count"] < rt.frame_noise_host(e["S"], e["Q"], 8)["count"], "the map's entries of 1 do not count"


def test_special_results_on_the_device(rt, gpu, inputs):
    one = inputs[(1, 1)]
    assert rt.frame_error(one["frame"], 1, one["ref"], 1)["psnr"] == mh.INF
    nothing = np.full((3, 5, 3), mh.NAN)
    assert rt.frame_error(nothing, 1, np.ones((3, 5, 3)), 1) == dict.fromkeys(mh.ERROR_FIELDS, 0.0) | {"count": 0}
    e = inputs[(257, 1)]
    assert rt.frame_noise(e["S"], e["Q"], 1) == dict(count=0, mean_var=0.0, noise=mh.INF, max_noise=mh.INF)


@pytest.mark.parametrize("w,h", [(257, 1), (257, 256)])
def test_inputs_and_the_bytes_around_the_workspace_are_left_alone_and_two_streams_agree(rt, gpu, inputs, w, h):
    import torch
    e = inputs[(w, h)]
    ws_bytes, guard = rt.metrics_workspace_bytes(w, h), 256
    host = {n: np.array(e[n]) for n in ("frame", "ref", "S", "Q")}
    d = {n: torch.from_numpy(a).cuda() for n, a in host.items()}
    d_map = torch.from_numpy(np.array(e["map"])).cuda()
    want_error = rt.frame_error_host(e["frame"], 1, e["ref"], 3, spp_map=e["map"])
    want_noise = rt.frame_noise_host(e["S"], e["Q"], 8)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, works = [], []
    torch.cuda.synchronize()
    for s in streams:
        d_ws = torch.full((ws_bytes + 2 * guard,), 0x5a, dtype=torch.uint8, device="cuda")   # (torch's allocations are 512-byte aligned)
        d_ws2 = torch.full((ws_bytes + 2 * guard,), 0x5a, dtype=torch.uint8, device="cuda")
        d_out8 = torch.full((8 + 2,), -7.0, dtype=torch.float64, device="cuda")
        d_out4 = torch.full((4 + 2,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rt.frame_error_device(w, h, d["frame"].data_ptr(), 1, d["ref"].data_ptr(), 3, d_out8.data_ptr() + 8, d_ws.data_ptr() + guard,
                              d_spp_ptr=d_map.data_ptr(), stream=s.cuda_stream)
        rt.frame_noise_device(w, h, "sums", d["S"].data_ptr(), d["Q"].data_ptr(), 8, d_out4.data_ptr() + 8, d_ws2.data_ptr() + guard,
                              stream=s.cuda_stream)
        outs.append((d_out8, d_out4))
        works.append((d_ws, d_ws2))
    torch.cuda.synchronize()
    for (d_out8, d_out4), pair in zip(outs, works):
        o8, o4 = d_out8.cpu().numpy(), d_out4.cpu().numpy()
        assert o8[0] == -7.0 and o8[-1] == -7.0 and o4[0] == -7.0 and o4[-1] == -7.0, "nothing around the outputs is written"
        assert mh.same_bits(dict(zip(mh.ERROR_FIELDS, o8[1:9])), want_error, mh.ERROR_FIELDS)
        assert mh.same_bits(dict(zip(mh.NOISE_FIELDS, o4[1:5])), want_noise, mh.NOISE_FIELDS)
        for d_ws in pair:
            raw = d_ws.cpu().numpy()
            assert (raw[:guard] == 0x5a).all() and (raw[guard + ws_bytes:] == 0x5a).all(), "bytes beyond the reported size are untouched"
    for n, a in host.items():
        assert np.array_equal(mh.bits(d[n].cpu().numpy()), mh.bits(a)), f"{n} is not written"
    assert np.array_equal(d_map.cpu().numpy(), e["map"])


@pytest.fixture(scope="module")
def scene(rt):
    hs = rt.HostScene(5, scene_seed=1, width=24, aspect=1.5, spp=12, depth=8)   # simple_light: the frame the tone-map test uses
    assert (hs.width, hs.height) == (24, 16)
    return hs, rt.DeviceScene(hs, device=0)


def test_a_real_render_against_itself_another_seed_and_its_own_moments(rt, gpu, scene):
    hs, ds = scene
    h, w = 16, 24
    sums = ds.render(rt.render_params(seed=3)).reshape(h, w, 3)
    same = rt.frame_error(sums, 12, sums, 12)
    assert same["count"] == w * h and same["psnr"] == mh.INF
    assert all(same[k] == 0.0 for k in ("mse", "rmse", "rel_mse", "mae", "bias", "max_abs"))
    ref = ds.render(rt.render_params(seed=4, sample_end=48)).reshape(h, w, 3)
    dev, host = rt.frame_error(sums, 12, ref, 48), rt.frame_error_host(sums, 12, ref, 48)
    assert mh.same_bits(dev, host, mh.ERROR_FIELDS) and mh.same_bits(dev, mh.frame_error(sums, 12, ref, 48), mh.ERROR_FIELDS)
    assert dev["mse"] > 0.0 and np.isfinite(dev["psnr"]) and dev["max_abs"] >= dev["mae"] > 0.0
    S, Q = ds.render_moments(rt.render_params(seed=3))
    assert np.array_equal(S, sums)
    dev, host = rt.frame_noise(S, Q, 12), rt.frame_noise_host(S, Q, 12)
    assert mh.same_bits(dev, host, mh.NOISE_FIELDS) and mh.same_bits(dev, mh.frame_noise(S, Q, 12), mh.NOISE_FIELDS)
    assert dev["count"] == w * h and 0.0 < dev["noise"] <= dev["max_noise"] < mh.INF
    M, M2 = ds.render_mean_moments(rt.render_params(seed=3))
    dev, host = rt.frame_noise(M, M2, 12, form="means"), rt.frame_noise_host(M, M2, 12, form="means")
    assert mh.same_bits(dev, host, mh.NOISE_FIELDS) and mh.same_bits(dev, mh.frame_noise(M, M2, 12, form="means"), mh.NOISE_FIELDS)
    assert dev["count"] == w * h and 0.0 < dev["noise"] < mh.INF


def test_render_until_stops_where_the_restatement_says(rt, gpu, scene):
    hs, ds = scene
    seed, min_samples, max_spp = 3, 5, 12
    # the noise after every pass of one sample, from render_mean_moments continued pass by pass, by the restatement (and the mirror)
    mean, m2, frames, noises = None, None, [], []
    for s in range(max_spp):
        mean, m2 = ds.render_mean_moments(rt.render_params(seed=seed, sample_begin=s, sample_end=s + 1), mean=mean, m2=m2)
        frames.append((mean.copy(), m2.copy()))
        want = mh.frame_noise(mean, m2, s + 1, form="means")
        assert mh.same_bits(rt.frame_noise_host(mean, m2, s + 1, form="means"), want, mh.NOISE_FIELDS)
        noises.append(want["noise"])
    assert noises[0] == mh.INF, "one sample says nothing"
    # a condition of the test, not a result: a pass strictly between min_samples and max_spp whose noise is below that of every
    # earlier pass from min_samples on — its noise is the threshold, so the loop must run past min_samples and stop there
    stop = next((n for n in range(min_samples + 1, max_spp) if noises[n - 1] < min(noises[min_samples - 1:n - 1])), None)
    assert stop is not None, noises
    threshold = noises[stop - 1]
    predicted = next(n for n in range(1, max_spp + 1) if (n >= min_samples and noises[n - 1] <= threshold) or n == max_spp)
    assert predicted == stop
    got_mean, got_m2, samples, noise = ds.render_until(threshold, max_spp=max_spp, min_samples=min_samples, seed=seed)
    assert samples == stop and mh.bits(noise) == mh.bits(threshold)
    assert np.array_equal(mh.bits(got_mean), mh.bits(frames[stop - 1][0])) and np.array_equal(mh.bits(got_m2), mh.bits(frames[stop - 1][1]))
    # a threshold nothing reaches: to max_spp, and the frames are render_mean_moments' at that count in one call
    got_mean, got_m2, samples, noise = ds.render_until(0.0, max_spp=max_spp, min_samples=min_samples, seed=seed)
    assert samples == max_spp and mh.bits(noise) == mh.bits(noises[-1])
    one_mean, one_m2 = ds.render_mean_moments(rt.render_params(seed=seed, sample_end=max_spp))
    assert np.array_equal(mh.bits(got_mean), mh.bits(one_mean)) and np.array_equal(mh.bits(got_m2), mh.bits(one_m2))
    # passes of several samples: the last one is cut at max_spp, and min_samples holds a low noise back
    got_mean, got_m2, samples, noise = ds.render_until(mh.INF, max_spp=11, pass_spp=4, min_samples=6, seed=seed)
    assert samples == 8 and mh.bits(noise) == mh.bits(noises[7])
    assert np.array_equal(mh.bits(got_mean), mh.bits(frames[7][0])) and np.array_equal(mh.bits(got_m2), mh.bits(frames[7][1]))
    assert ds.render_until(0.0, max_spp=11, pass_spp=4, seed=seed)[2] == 11
