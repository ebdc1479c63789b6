"""The scheduler thresholds and the job hand-out "affect speed only, never results" (rt_amd.h, rt_amd_debug.h): held here on every class
of render kernel, in all three job modes, against the CPU oracle.

path_kernel is a wave-scheduled megakernel: which stage runs next, and so what every lane has in flight when — the per-path RNG, parked
attenuations, instances waiting in a bit mask, lanes queued with a dear texture, the merged path end — follows from five thresholds, and
which wave traces which job from the guided hand-out.  The presets produce ONE schedule per kernel; a change that is right under it and
wrong under another passes every test that renders under the presets.  tests/schedule_cases.py lists the settings, what each forces,
and why none of them can stall a wave (read from the scheduler's code before anything ran: no setting was dropped).

Every expected frame is the oracle's frame of the same scene, camera, seed and sample range, compared as u64 — never a device render
under another setting.  Thresholds reach a scene through its own options (rt_scene_options.th_*) only.

1. Threshold matrix, dense mode: every class of tests/kernel_classes.py under nine settings (thresholds 0, 1, 64, 255; both path ends),
   the classes with textures under two more (slow lanes that wait for ever / never).  rt_debug_last_kernel must still report the class.
2. List and views modes on every class under lazy_split and eager_merged, with test_gpu_job_modes.py's harness and assertions.
3. The counted kernel (its own instantiation) on one class per feature set: the frame, the path-determined counters identical under
   every setting — node_visits among them: a walk's visits depend on the lane's own ray and interval only (any_degenerate is a ballot,
   but wide_verdict uses it only to skip work for lanes that are not degenerate) —, and, from rt_debug_stage_profile, the proof that
   the setting reached the kernel: new-job rounds exactly where th_new > 0, another number of rounds under `phases`.
4. RT_JOBS_PER_GRAB / RT_GRAB_TAPER, read when the library loads: one child process per setting, one after the other.  The large frame
   (400x225, 10 spp: 1450 tiles x 64 x 10 = 928 000 jobs) is launched with ceil(928 000 / (256 x 16)) = 227 workgroups of 16 waves, 3632
   waves; under RT_GRAB_TAPER=1 a wave's first grab is trunc(928 000 / 3632 = 255.5) rounded down to a multiple of 64: 192, strictly
   between the minimum of 128 and the 1024 asked for, so taper 1 it is.  The test does this arithmetic on the launch the child reports.
5. Frames of 1x1, 3x2, 8x8 and 9x8 pixels at 1 and 3 spp (64 jobs, half a minimum grab, and up), and paths of depth 1 and 2.  Neither
   the host library nor scene creation refuses any of these sizes.

Added GPU time, measured on an MI355X: 29.5 s for the file run alone (483 cases).  11.4 s of it are the process's first use of torch and
its device context (here the first list-mode case, not the file's first case; within the whole suite that is paid once anyway) and
12.8 s the three child processes, 4.1 to 4.4 s each, nearly all of it their own start of Python, torch and the device.  No other case
takes more than 0.21 s (a scene creation with 65 535 materials).  The oracle's 144 frames take 0.63 s of it on 16 CPU cores; the 400x225 frame
at 10 spp is the largest of them."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import denoise_helpers
import kernel_classes as kc
import scene_cases
import schedule_cases as sc
from adaptive_helpers import SENTINEL, assert_bits, bits
from job_mode_helpers import LIST_SEED, VIEWS_SEED, check_listed, listed, oracle_moments, oracle_sum, oracle_views, views_on_device
from live_helpers import oracle_samples

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TEXTURED = [c for c, (_, _, k) in kc.CLASSES.items() if k["features"] & sc.FEAT_TEXTURES]

_depth_frames, _handout_want = {}, {}


def check_frame(got, want, what):
    assert np.isfinite(want).all() and want.any(), f"{what}: the oracle's frame is no test"
    assert np.isfinite(got).all() and got.any(), f"{what}: the frame is not finite or all zero"
    assert_bits(got, want, what)


def dense_under(rt, cls, setting, params):
    """the class's scene created under the setting and rendered once, dense; the launch must be the class's kernel"""
    ds = kc.device_scene(rt, cls, **sc.options(setting))
    try:
        got = ds.render(params)
        assert rt.debug_last_kernel() == kc.expected_kernel(cls, 0), (cls, setting)
        kc.check_stats(cls, ds.stats())
    finally:
        ds.close()
    return got


# ---------------- 1. the threshold matrix, dense mode ----------------

def matrix_case(rt, oracle, cls, setting):
    name = kc.CLASSES[cls][0]
    n = kc.spp_of(name)
    got = dense_under(rt, cls, setting, rt.render_params(seed=LIST_SEED, sample_end=n))
    check_frame(got, oracle_sum(rt, oracle, name, n), f"{cls} under {setting}")


@pytest.mark.parametrize("setting", list(sc.SETTINGS))
@pytest.mark.parametrize("cls", list(kc.CLASSES))
def test_dense_frame_under_thresholds(rt, oracle, gpu, cls, setting):
    matrix_case(rt, oracle, cls, setting)


@pytest.mark.parametrize("setting", list(sc.TEXTURE_SETTINGS))
@pytest.mark.parametrize("cls", TEXTURED)
def test_dense_frame_with_slow_lanes_queued(rt, oracle, gpu, cls, setting):
    matrix_case(rt, oracle, cls, setting)


def test_the_matrix_flips_every_preset_and_reaches_the_texture_kernels():
    assert sc.th_new_of("new_merged") == 0 and sc.th_new_of("new_split") > 0
    assert {kc.CLASSES[c][2]["features"] for c in TEXTURED} == {kc.FEAT["spheres_quads_textures"], kc.FEAT["all"]}
    assert all(0 <= v <= 255 for s in sc.SETTINGS.values() for v in s if v >= 0)  # (the kernel takes four of them as bytes)


# ---------------- 2. list and views modes ----------------

@pytest.mark.parametrize("setting", ["lazy_split", "eager_merged"])
@pytest.mark.parametrize("cls", list(kc.CLASSES))
def test_list_mode_under_thresholds(rt, oracle, gpu, cls, setting):
    name = kc.CLASSES[cls][0]
    hs, n = kc.scene(rt, name), kc.spp_of(name)
    pixels, chosen = kc.stress_list(hs.width * hs.height)
    ds = kc.device_scene(rt, cls, **sc.options(setting))
    try:
        got, got_sq, _ = listed(rt, ds, hs, pixels, [(0, n)])
        assert rt.debug_last_kernel() == kc.expected_kernel(cls, kc.JOBS_LIST), (cls, setting)
        kc.check_stats(cls, ds.stats())
    finally:
        ds.close()
    total, s, q = oracle_moments(rt, oracle, name, n)
    assert_bits(s, total, "oracle: the in-order sum of its single samples against its own range render")
    check_listed(got, got_sq, chosen, total, q, f"{cls} under {setting}")


@pytest.mark.parametrize("setting", ["lazy_split", "eager_merged"])
@pytest.mark.parametrize("cls", list(kc.CLASSES))
def test_views_mode_under_thresholds(rt, oracle, gpu, cls, setting):
    name = kc.CLASSES[cls][0]
    n = kc.spp_of(name)
    views = kc.three_views(rt, name, VIEWS_SEED)
    ds = kc.device_scene(rt, cls, **sc.options(setting))
    try:
        got, guards = views_on_device(rt, ds, views, n)
        assert rt.debug_last_kernel() == kc.expected_kernel(cls, kc.JOBS_VIEWS), (cls, setting)
        kc.check_stats(cls, ds.stats())
        assert rt.debug_last_launch()["launches"] == 1
    finally:
        ds.close()
    for v, want in enumerate(oracle_views(rt, oracle, name, views, n)):
        assert_bits(got[v], want, f"{cls} under {setting}: view {v} of 3")
    assert (bits(guards) == SENTINEL).all(), f"{cls} under {setting}: the doubles before or after d_out were written"


# ---------------- 3. the counted kernel ----------------

COUNTED = ["spheres_solid-lds3-own-wide1", "quads_frames-lds3-own-wide0", "quads_frames_media-lds3-own",
           "textures-lds3-ref-two_perlin_spheres", "all-lds3-own-wide1-textured_frames", "all-lds0-media-sequence"]
COUNTED_SETTINGS = ["preset", "eager_split", "lazy_merged", "phases"]
PATH_COUNTERS = ["samples", "rays", "rng_draws", "sphere_tests", "quad_tests", "medium_visits", "noise_evals", "image_lookups",
                 "instance_enters", "node_visits"]
STAGES = ["box", "sphere", "quad", "other", "shade", "newjob"]


def preset_splits_the_path_end(cls):
    """rt_scene_plan.hpp Tuning: of the presets these classes get, only the spheres-only kernel's has th_new > 0 (spheres_solid 28;
    quads_frames — the Cornell box has instances —, ordered_general, ordered_global and general have 0)"""
    return kc.CLASSES[cls][2]["features"] == kc.FEAT["spheres_solid"]


@pytest.mark.parametrize("cls", COUNTED)
def test_counted_kernel_under_thresholds(rt, oracle, gpu, cls):
    import torch
    name = kc.CLASSES[cls][0]
    hs, n = kc.scene(rt, name), kc.spp_of(name)
    want = oracle_sum(rt, oracle, name, n)
    counters, rounds = {}, {}
    for setting in COUNTED_SETTINGS:
        ds = kc.device_scene(rt, cls, **sc.options(setting))
        try:
            d = torch.zeros(hs.width * hs.height * 3, dtype=torch.float64, device="cuda")
            counters[setting] = ds.render_device_counted(rt.render_params(seed=LIST_SEED, sample_end=n), d.data_ptr(),
                                                         torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rt.debug_last_kernel() == kc.expected_kernel(cls, 0), (cls, setting)
            profile = rt.debug_stage_profile()
        finally:
            ds.close()
        rounds[setting] = {s: profile[s]["rounds"] for s in STAGES}
        print(cls, setting, counters[setting], rounds[setting])
        check_frame(d.cpu().numpy(), want, f"{cls} counted under {setting}")
    assert counters["preset"]["samples"] == hs.width * hs.height * n and counters["preset"]["rays"] >= counters["preset"]["samples"]
    for setting in COUNTED_SETTINGS[1:]:
        for key in PATH_COUNTERS:
            assert counters[setting][key] == counters["preset"][key], (cls, setting, key, counters[setting][key], counters["preset"][key])
    # the setting reached the kernel: separate path-end rounds exactly where th_new > 0 ...
    for setting in COUNTED_SETTINGS:
        th_new = sc.th_new_of(setting)
        split = preset_splits_the_path_end(cls) if th_new is None else th_new > 0
        assert (rounds[setting]["newjob"] > 0) == split, (cls, setting, rounds[setting])
        assert rounds[setting]["shade"] > 0 and rounds[setting]["box"] > 0, (cls, setting, rounds[setting])
    # ... and another schedule altogether under `phases`
    assert sum(rounds["phases"].values()) != sum(rounds["preset"].values()), (cls, rounds)


# ---------------- 4. the job hand-out ----------------

def handout_want(rt, oracle):
    """the oracle's frames of what a child renders, once for the three children"""
    if _handout_want:
        return _handout_want
    w = {}
    for name in sc.DENSE + (sc.LARGE,):
        hs = scene_cases.build(rt, name)
        w["dense--" + name] = oracle.render(hs, rt.render_params(seed=sc.HANDOUT_SEED))
        if name == sc.RAGGED:
            w["tiles--" + name] = oracle.render(hs, rt.render_params(seed=sc.HANDOUT_SEED, out_layout=rt.RT_OUT_TILES, **sc.SHARD))
            n, n_pix = hs.camera.samples_per_pixel, hs.width * hs.height
            _, q = denoise_helpers.moments(oracle_samples(rt, oracle, hs, n, LIST_SEED), (n_pix, 3))
            w["list--" + name] = oracle.render(hs, rt.render_params(seed=LIST_SEED, sample_end=n)).reshape(n_pix, 3)
            w["list_sq--" + name] = q
            w["chosen"] = kc.stress_list(n_pix)[1]
        if name == sc.LARGE:
            w["large_tiles"] = ((hs.width + 7) // 8) * ((hs.height + 7) // 8)
            w["large_spp"] = hs.camera.samples_per_pixel
    views = kc.three_views(rt, sc.VIEWS_SCENE, VIEWS_SEED)
    w["views"] = oracle_views(rt, oracle, sc.VIEWS_SCENE, views, kc.spp_of(sc.VIEWS_SCENE))
    _handout_want.update(w)
    return _handout_want


@pytest.mark.parametrize("handout", list(sc.HANDOUTS))
def test_job_handout_settings_change_no_frame(rt, oracle, gpu, tmp_path, handout):
    per_grab, taper = sc.HANDOUTS[handout]
    env = {k: v for k, v in os.environ.items() if k not in ("RT_JOBS_PER_GRAB", "RT_GRAB_TAPER")}
    if per_grab is not None:
        env["RT_JOBS_PER_GRAB"] = str(per_grab)
    env["RT_GRAB_TAPER"] = str(taper)
    out = str(tmp_path / "frames.npz")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "schedule_cases.py"), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (handout, r.returncode, r.stderr[-2000:])
    launch = json.loads(r.stdout.strip().splitlines()[-1])["launch"]
    got = np.load(out)
    want = handout_want(rt, oracle)

    # the large frame's launch, and the first grab it leads to: 1024 without the taper, strictly inside (128, 1024) with it, 128 under
    # a taper that leaves less than the minimum
    assert launch["launches"] == 1, launch
    waves = launch["grid"] * launch["threads"] // 64
    first = sc.first_grab(want["large_tiles"] * 64 * want["large_spp"], waves, per_grab or 0, taper)
    print(handout, launch, "waves", waves, "first grab", first)
    if handout == "grab1024-taper0":
        assert first == sc.MAX_JOBS_PER_GRAB
    elif handout == "grab1024-taper1":
        assert sc.MIN_JOBS_PER_GRAB < first < sc.MAX_JOBS_PER_GRAB, (launch, first)
    else:
        assert first == sc.MIN_JOBS_PER_GRAB

    for name in sc.DENSE + (sc.LARGE,):
        check_frame(got["dense--" + name], want["dense--" + name], f"{handout}: {name}")
    check_frame(got["tiles--" + sc.RAGGED], want["tiles--" + sc.RAGGED], f"{handout}: {sc.RAGGED}, shard 1 of 3 in tiles layout")
    check_listed(got["list--" + sc.RAGGED], got["list_sq--" + sc.RAGGED], want["chosen"], want["list--" + sc.RAGGED],
                 want["list_sq--" + sc.RAGGED], f"{handout}: list mode on {sc.RAGGED}")
    for v, frame in enumerate(want["views"]):
        assert_bits(got["views"][v], frame, f"{handout}: view {v} of 3")
    assert (bits(got["guards"]) == SENTINEL).all(), f"{handout}: the doubles before or after the views' frames were written"


# ---------------- 5. frames smaller than a grab, and the shortest paths ----------------

SMALL_SEED = 5


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("size", [(1, 1), (3, 2), (8, 8), (9, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scene", [0, 6], ids=["random_spheres", "cornell_box"])
def test_frames_smaller_than_a_grab(rt, oracle, gpu, scene, size, spp):
    """n_jobs = tiles x 64 x spp = 64, 128, 192 or 384: one workgroup, whose first grab (128 at least) reaches past the end for the
    first two.  (The Cornell box's single pixel is black at these sample counts: there the frame is held to the oracle's zeros.)"""
    w, h = size
    hs = rt.HostScene(scene, width=w, aspect=w / h, spp=spp, depth=50)
    assert (hs.width, hs.height) == (w, h)
    params = rt.render_params(seed=SMALL_SEED)
    want = oracle.render(hs, params)
    assert np.isfinite(want).all() and (want.any() or (scene == 6 and size == (1, 1)))
    for setting in ("preset", "lazy_split", "eager_merged"):
        ds = rt.DeviceScene(hs, **sc.options(setting))
        try:
            got = ds.render(params)
            launch = rt.debug_last_launch()
        finally:
            ds.close()
        assert (launch["launches"], launch["grid"]) == (1, 1), launch
        assert_bits(got, want, f"scene {scene} at {w}x{h}, {spp} spp under {setting}")


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("cls", ["spheres_solid-lds3-own-wide1", "quads_frames-lds3-own-wide0", "all-lds3-own-media", "colour_parking-lds3-own"])
def test_the_shortest_paths(rt, oracle, gpu, cls, depth):
    """max_depth 1: every path ends at its first hit (a light, else zero) or on the background, with nothing parked but a light's
    colour; 2: one attenuation at most"""
    name = kc.CLASSES[cls][0]
    n = kc.spp_of(name)
    params = rt.render_params(seed=LIST_SEED, sample_end=n, max_depth=depth)
    if (name, depth) not in _depth_frames:
        f = oracle.render(kc.scene(rt, name), params)
        f.setflags(write=False)
        _depth_frames[name, depth] = f
    for setting in ("preset", "new_split", "new_merged"):
        check_frame(dense_under(rt, cls, setting, params), _depth_frames[name, depth], f"{cls} at depth {depth} under {setting}")
