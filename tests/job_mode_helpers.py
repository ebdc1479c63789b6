"""Shared by tests/test_gpu_job_modes.py and tests/test_gpu_schedule.py (not a test module): the list-mode and views-mode harness on the
scenes of tests/kernel_classes.py, and the CPU oracle's frames of those scenes, rendered once per process and left unchanged.

List mode: rt_render_pixels_device with d_sum_sq onto sentinel-filled frames (`listed`, `check_listed`); views mode:
rt_render_views_device into the middle of a sentinel-filled buffer (`views_on_device`).  The oracle's frames are cached in module-level
dictionaries per (scene, sample count) and per (scene, camera, seed, sample count), so that a further setting of the same scene costs a
scene creation and a render only."""
import numpy as np

import denoise_helpers
import kernel_classes as kc
from adaptive_helpers import SENTINEL, assert_bits, bits
from live_helpers import oracle_samples

LIST_SEED, VIEWS_SEED = 3, 11
GUARD = 1024     # doubles before and after the views' frames

_samples, _sums, _view_frames = {}, {}, {}


def oracle_sum(rt, oracle, name, n):
    """the oracle's own frame of sums over [0, n) under the scene's camera and LIST_SEED, flat (read-only)"""
    if (name, n) not in _sums:
        total = oracle.render(kc.scene(rt, name), rt.render_params(seed=LIST_SEED, sample_end=n))
        total.setflags(write=False)
        _sums[name, n] = total
    return _sums[name, n]


def oracle_moments(rt, oracle, name, n):
    """(the oracle's own sums over [0, n), the in-order sums of its single-sample frames, the in-order sums of their squares), each
    (n_pix, 3), under the scene's camera and LIST_SEED"""
    hs = kc.scene(rt, name)
    have = _samples.setdefault(name, [])
    if len(have) < n:
        have[:] = oracle_samples(rt, oracle, hs, n, LIST_SEED)
    n_pix = hs.width * hs.height
    s, q = denoise_helpers.moments(have[:n], (n_pix, 3))
    return oracle_sum(rt, oracle, name, n).reshape(n_pix, 3), s, q


def oracle_views(rt, oracle, name, views, n):
    out = []
    for v in views:
        key = (name, bytes(v.camera), int(v.seed), n)
        if key not in _view_frames:
            f = oracle.render(kc.scene(rt, name), rt.render_params(seed=int(v.seed), sample_end=n),
                              camera=rt.Camera.from_buffer_copy(bytes(v.camera)))
            f.setflags(write=False)
            _view_frames[key] = f
        out.append(_view_frames[key])
    assert len({bits(f).tobytes() for f in out}) == len(out), "two views have the same oracle frame: the case checks less than it says"
    return out


def listed(rt, ds, hs, pixels, ranges):
    """rt_render_pixels_device with d_sum_sq over each (begin, end) in turn — the first onto sentinel-filled frames, the later ones
    with accumulate — and the launch counts; returns the two frames as (n_pix, 3)"""
    import torch
    n_pix = hs.width * hs.height
    lst = torch.from_numpy(pixels.view(np.int32)).cuda()
    s = torch.full((n_pix * 3,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
    q = torch.full((n_pix * 3,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
    launches = []
    for b, e in ranges:
        ds.render_pixels_device(rt.render_params(seed=LIST_SEED, sample_begin=b, sample_end=e, accumulate=b > ranges[0][0]),
                                lst.data_ptr(), len(pixels), s.data_ptr(), q.data_ptr(), torch.cuda.current_stream().cuda_stream)
        launches.append(rt.debug_last_launch()["launches"])
    torch.cuda.synchronize()
    return s.cpu().numpy().reshape(n_pix, 3), q.cpu().numpy().reshape(n_pix, 3), launches


def check_listed(got, got_sq, chosen, want, want_sq, what):
    mask = np.zeros(got.shape[0], dtype=bool)
    mask[chosen] = True
    assert_bits(got[mask], want[mask], f"{what}: sums of the listed pixels")
    assert_bits(got_sq[mask], want_sq[mask], f"{what}: squared sums of the listed pixels")
    assert (bits(got[~mask]) == SENTINEL).all() and (bits(got_sq[~mask]) == SENTINEL).all(), f"{what}: an unlisted pixel was written"


def views_on_device(rt, ds, views, n):
    """rt_render_views_device into the middle of a sentinel-filled buffer; returns (frames (3, frame), the guards before and after)"""
    import torch
    frame = views[0].camera.image_width * views[0].camera.image_height * 3
    d = torch.full((GUARD + len(views) * frame + GUARD,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
    ds.render_views_device(rt.render_params(sample_end=n), views, d[GUARD:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    return out[GUARD:-GUARD].reshape(len(views), frame), np.concatenate([out[:GUARD], out[-GUARD:]])
