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

import pytest

import kernel_classes as kc
from adaptive_helpers import SENTINEL, assert_bits, bits, check_adaptive_against_oracle, launches_for
from job_mode_helpers import LIST_SEED, VIEWS_SEED, check_listed, listed, oracle_moments, oracle_views, views_on_device

pytestmark = pytest.mark.gpu

N_MULTI = 6      # samples of the several-launch cases

_device = {}


def device_scene(rt, cls):
    """one DeviceScene per class, shared by its list and its views case"""
    if cls not in _device:
        _device[cls] = kc.device_scene(rt, cls)
    return _device[cls]


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
