"""List mode (rt_render_pixels_device; path_kernel<..., JOBS_LIST>) and views mode (rt_render_views_device; JOBS_VIEWS) on every class
of render kernel: each combination of LDS level, feature set, walk, record width and AUX that path_kernel_for picks is a code object
of its own, with its own registers and launch set-up, and either job mode doubles the table (tests/kernel_classes.py lists the
classes and the smallest scene found for each).

Every case renders one scene in one class.  Its first assertion is on rt_debug_last_kernel: the launch really was that class and
that mode (a scene that lands in a neighbouring cell fails, it does not skip); DeviceScene.stats() confirms the walk and the LDS
image.  The frames are then held, as u64, to the CPU oracle's frames of the same scene, camera, seed and sample range — never to
the dense device render, which is code under test here.

List mode, one stress shape for every class: a shuffled 60 % of the pixels with padding entries at random places, a length that is no
multiple of 64, frames pre-filled with a sentinel; the listed pixels equal the oracle's sums and the in-order sums of the squares of
the oracle's single-sample frames, every other value is still the sentinel, and [0, n/2) followed by [n/2, n) with accumulate equals
the single call.  Views mode: three views with their own cameras and seeds, the middle one without defocus between two with; 25 tiles
(or 16, or 15) per view, so view boundaries fall inside a wave's grab; guard doubles before and after d_out stay untouched.

Not reachable by any scene: LDS level 2 (path_kernel_for has it, scene creation never chooses it).

Added GPU time, measured on an MI355X: 13.9 s for the file run alone (62 cases), 11.1 s of it in the first case (the process's first
use of the device and of torch; within the whole suite that is paid once anyway), no other case above 0.7 s.  The oracle's frames
of all 12 scenes take 0.6 s of it on 16 CPU cores (3.5 s on 8); the 6000-sphere flat list at 37x37 is the largest job."""
import os

import numpy as np
import pytest

import denoise_helpers
import kernel_classes as kc
from adaptive_helpers import SENTINEL, assert_bits, bits, check_adaptive_against_oracle, launches_for
from live_helpers import oracle_samples

pytestmark = pytest.mark.gpu

LIST_SEED, VIEWS_SEED = 3, 11
N_MULTI = 6      # samples of the several-launch cases
GUARD = 1024     # doubles before and after the views' frames

_device, _samples, _sums, _view_frames = {}, {}, {}, {}


def device_scene(rt, cls):
    """one DeviceScene per class, shared by its list and its views case"""
    if cls not in _device:
        _device[cls] = kc.device_scene(rt, cls)
    return _device[cls]


def oracle_moments(rt, oracle, name, n):
    """(the oracle's own sums over [0, n), the in-order sums of its single-sample frames, the in-order sums of their squares), each
    (n_pix, 3), under the scene's camera and LIST_SEED"""
    hs = kc.scene(rt, name)
    have = _samples.setdefault(name, [])
    if len(have) < n:
        have[:] = oracle_samples(rt, oracle, hs, n, LIST_SEED)
    if (name, n) not in _sums:
        total = oracle.render(hs, rt.render_params(seed=LIST_SEED, sample_end=n))
        total.setflags(write=False)
        _sums[name, n] = total
    n_pix = hs.width * hs.height
    s, q = denoise_helpers.moments(have[:n], (n_pix, 3))
    return _sums[name, n].reshape(n_pix, 3), s, q


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


@pytest.mark.parametrize("cls", list(kc.CLASSES))
def test_list_mode_equals_the_oracle(rt, oracle, gpu, cls):
    name = kc.CLASSES[cls][0]
    hs, ds, n = kc.scene(rt, name), device_scene(rt, cls), kc.spp_of(name)
    pixels, chosen = kc.stress_list(hs.width * hs.height)
    got, got_sq, _ = listed(rt, ds, hs, pixels, [(0, n)])
    assert rt.debug_last_kernel() == kc.expected_kernel(cls, kc.JOBS_LIST), cls
    kc.check_stats(cls, ds.stats())
    total, s, q = oracle_moments(rt, oracle, name, n)
    assert_bits(s, total, "oracle: the in-order sum of its single samples against its own range render")
    check_listed(got, got_sq, chosen, total, q, cls)
    both, both_sq, _ = listed(rt, ds, hs, pixels, [(0, n // 2), (n // 2, n)])
    assert_bits(both, got, f"{cls}: [0, {n // 2}) + [{n // 2}, {n}) with accumulate against one call, sums")
    assert_bits(both_sq, got_sq, f"{cls}: [0, {n // 2}) + [{n // 2}, {n}) with accumulate against one call, squared sums")


@pytest.mark.parametrize("cls", list(kc.CLASSES))
def test_views_mode_equals_the_oracle(rt, oracle, gpu, cls):
    name = kc.CLASSES[cls][0]
    ds, n = device_scene(rt, cls), kc.spp_of(name)
    views = kc.three_views(rt, name, VIEWS_SEED)
    got, guards = views_on_device(rt, ds, views, n)
    assert rt.debug_last_kernel() == kc.expected_kernel(cls, kc.JOBS_VIEWS), cls
    kc.check_stats(cls, ds.stats())
    assert rt.debug_last_launch()["launches"] == 1
    for v, want in enumerate(oracle_views(rt, oracle, name, views, n)):
        assert_bits(got[v], want, f"{cls}: view {v} of 3")
    assert (bits(guards) == SENTINEL).all(), f"{cls}: the doubles before or after d_out were written"


def test_the_classes_cover_both_values_of_aux():
    on = [c for c, (_, _, k) in kc.CLASSES.items() if k["ordered"] and k["aux"]]
    off = [c for c, (_, _, k) in kc.CLASSES.items() if k["ordered"] and not k["aux"]]
    assert on and off, (on, off)


def overlap():
    return os.environ.get("RT_OVERLAP", "1") != "0"


@pytest.mark.parametrize("cls", ["all-lds1-own-wide1", "all-lds0-media-sequence"])
def test_a_list_render_of_several_launches(rt, oracle, gpu, cls):
    """a sample buffer of two and a half sample rows of the list: N_MULTI samples take N_MULTI launches over two scratch sets (three
    launches of two samples with RT_OVERLAP=0)"""
    name = kc.CLASSES[cls][0]
    hs = kc.scene(rt, name)
    pixels, chosen = kc.stress_list(hs.width * hs.height)
    budget = ((len(pixels) + 63) // 64) * 64 * 24 * 5 // 2
    want_launches = launches_for(len(pixels), N_MULTI, budget, overlap())[0]
    assert want_launches >= 3
    ds = kc.device_scene(rt, cls, sample_buffer_bytes=budget)
    got, got_sq, launches = listed(rt, ds, hs, pixels, [(0, N_MULTI)])
    assert rt.debug_last_kernel() == kc.expected_kernel(cls, kc.JOBS_LIST), cls
    assert launches == [want_launches]
    total, s, q = oracle_moments(rt, oracle, name, N_MULTI)
    assert_bits(s, total, "oracle: the in-order sum of its single samples against its own range render")
    check_listed(got, got_sq, chosen, total, q, f"{cls}, {want_launches} launches")


@pytest.mark.parametrize("cls", ["all-lds1-ref", "all-lds0-own-wide0"])
def test_a_views_render_of_several_launches(rt, oracle, gpu, cls):
    """a sample buffer of two and a half sample rows of the three views' tiles"""
    name = kc.CLASSES[cls][0]
    hs = kc.scene(rt, name)
    views = kc.three_views(rt, name, VIEWS_SEED)
    entries = 3 * ((hs.width + 7) // 8) * ((hs.height + 7) // 8) * 64
    budget = entries * 24 * 5 // 2
    want_launches = launches_for(entries, N_MULTI, budget, overlap())[0]
    assert want_launches >= 3
    ds = kc.device_scene(rt, cls, sample_buffer_bytes=budget)
    got, guards = views_on_device(rt, ds, views, N_MULTI)
    assert rt.debug_last_kernel() == kc.expected_kernel(cls, kc.JOBS_VIEWS), cls
    assert rt.debug_last_launch()["launches"] == want_launches
    for v, want in enumerate(oracle_views(rt, oracle, name, views, N_MULTI)):
        assert_bits(got[v], want, f"{cls}, {want_launches} launches: view {v} of 3")
    assert (bits(guards) == SENTINEL).all()


def test_adaptive_render_with_the_records_in_the_lds(rt, oracle, gpu):
    """rt_render_adaptive end to end on the 1200-sphere scene (LDS level 1, four-child records): points 4, 8, 12 at rel 0.25, abs 0.02.
    Under the ORACLE's sums 67.3 % of the pixels stop at 4 samples, 13.7 % at 8 and 19.1 % at 12 (921, 187 and 261 of 1369):
    check_adaptive_against_oracle holds the schedule to at least 5 % at three points before it renders."""
    cls = "all-lds1-own-wide1"
    hs, ds = kc.scene(rt, kc.CLASSES[cls][0]), device_scene(rt, cls)
    want_spp = check_adaptive_against_oracle(rt, oracle, hs, ds, min_spp=4, batch=4, max_spp=12, rel=0.25, abs_=0.02, seed=LIST_SEED, min_share=0.05)
    assert rt.debug_last_kernel() == kc.expected_kernel(cls, kc.JOBS_LIST)
    assert [int((want_spp == nk).sum()) for nk in (4, 8, 12)] == [921, 187, 261]
