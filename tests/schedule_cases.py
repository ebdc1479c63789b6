"""Shared by tests/test_gpu_schedule.py (not a test module): the scheduler settings of its threshold matrix, the arithmetic of the
guided job hand-out, and the program its child processes run.

A setting is (th_prim, th_other, th_shade, th_box, th_new) in 64ths of a wave's live lanes, -1 for the kernel's preset; it reaches a
scene through the per-scene options only (rt_scene_options.th_*), never through the process-wide rt_debug_set_tuning.  What each
forces is read from path_kernel's scheduler (rt_kernel.hip, "scheduler: which stage has enough lanes queued?"): a deferred stage with c
lanes queued is runnable by count when c * 64 >= th * live and c > 0, the largest runnable queue wins, the box stage runs when none is
and a lane walks, and when no lane walks and no count suffices the largest queue runs all the same; the box loop goes on while
in_box * 64 >= th_box * live and in_box > 0; th_new == 0 merges the path end into the shade rounds.

    eager_merged   any non-empty queue is runnable, the largest wins; the box loop runs until no lane walks; merged path end
    eager_split    the same with new-job rounds of their own as soon as one lane waits
    full_wave      a stage runs by count only when every live lane waits for it
    lazy_split     no count ever suffices (c * 64 >= 255 * live is impossible): stages run only when nothing else can, one box round per pass
    lazy_merged    the same with the merged path end
    phases         the box loop runs until every walking lane has left it, only then the largest other queue: every leaf and every shade
                   waits as long as it can
    box_starved    everything else eager, one box round per pass
    new_merged, new_split    the presets with one or the other path end: for every class one of the two flips the preset's

(lazy_merged and phases come to nearly the same schedule: with no count ever sufficient the box stage is chosen again pass after pass
while a lane walks, which is what phases' box loop does in one pass.  The counted kernel reports the same rounds per stage for the two
on the kernels without instances, and a fraction of a per cent apart on the others, where a pass's start hands out deferred instances.)

None of them can leave a pass of the scheduler without progress: with a live lane either a deferred queue is non-empty and chosen (by
count, or by the "nothing else can run" rule, which needs no count), or a lane walks and the box stage runs, whose loop is a do-while: one
round at least.  A chosen stage advances every lane queued for it but the shade stage's lanes with a dear texture, and those go ahead
when they are the round's only lanes (`n_slow == popcount(ballot(true))`) whatever slow_min and slow_age say; a new-job round hands out
a job or, when none is left, retires the lane."""
import json
import sys
from pathlib import Path

import numpy as np

SETTINGS = {
    "eager_merged": (0, 0, 0, 0, 0),
    "eager_split": (0, 0, 0, 0, 1),
    "full_wave": (64, 64, 64, 64, 64),
    "lazy_split": (255, 255, 255, 255, 255),
    "lazy_merged": (255, 255, 255, 255, 0),
    "phases": (255, 255, 255, 0, 0),
    "box_starved": (1, 1, 1, 255, 1),
    "new_merged": (-1, -1, -1, -1, 0),
    "new_split": (-1, -1, -1, -1, 16),
}
# for the kernels with textures: the shade stage's queue of lanes with a dear texture (KParams::slow_min, slow_age)
TEXTURE_SETTINGS = {
    "lazy_split-slow_wait": ("lazy_split", dict(slow_min=64, slow_age=1 << 20)),  # a slow lane waits until only slow lanes shade
    "eager_merged-slow_min1": ("eager_merged", dict(slow_min=1)),                 # nobody waits
}
FEAT_TEXTURES = 16  # rt_kernels.h: the bit of a kernel's feature mask


def options(setting):
    """the rt_scene_options fields of a setting ("preset": none)"""
    if setting == "preset":
        return {}
    more = {}
    if setting in TEXTURE_SETTINGS:
        setting, more = TEXTURE_SETTINGS[setting]
    return dict(zip(("th_prim", "th_other", "th_shade", "th_box", "th_new"), SETTINGS[setting]), **more)


def th_new_of(setting):
    """a setting's th_new, None where it is the preset's"""
    v = options(setting).get("th_new", -1)
    return None if v < 0 else v


# ---- the guided job hand-out (rt_api.cpp launch_render "~32 grabs per wave or more", rt_kernel.hip "guided hand-out") ----
MAX_JOBS_PER_GRAB, MIN_JOBS_PER_GRAB = 1024, 128   # rt_kernels.h

# RT_JOBS_PER_GRAB, RT_GRAB_TAPER (None: not set; the library's defaults are 0 — ~32 grabs per wave — and 8)
HANDOUTS = {
    "grab1024-taper0": (1024, 0),     # fixed large grabs, no taper: on the small frames the first round of grabs reaches past n_jobs
    "grab1024-taper1": (1024, 1),     # the taper is active: grabs between the two limits that shrink as the launch runs out
    "taper4096": (None, 4096),        # every grab is the minimum
}


def first_grab(n_jobs, waves, jobs_per_grab, grab_taper):
    """The size of a wave's first grab, in the host's and the kernel's own arithmetic: jobs_per_grab is RT_JOBS_PER_GRAB or
    n_jobs / (32 waves), rounded down to a multiple of 64 within [MIN, MAX]; the taper factor is 1 / (waves x RT_GRAB_TAPER) in f32 (1
    with the taper off); the grab is trunc(f32(jobs left) x factor) rounded down to a multiple of 64, at most jobs_per_grab, at least MIN."""
    per_grab = jobs_per_grab if jobs_per_grab else n_jobs // (waves * 32)
    per_grab = min(max(per_grab // 64 * 64, MIN_JOBS_PER_GRAB), MAX_JOBS_PER_GRAB)
    factor = np.float32(1.0) / np.float32(waves * grab_taper) if grab_taper > 0 else np.float32(1.0)
    grab = int(np.float32(n_jobs) * factor) & ~63
    return max(min(grab, per_grab), MIN_JOBS_PER_GRAB)


HANDOUT_SEED = 4
DENSE = ("c2_random_balls_96x64_8spp_d50", "cornell_smoke_64x64_16spp", "ragged_random_balls_53x29_4spp")
RAGGED, LARGE = "ragged_random_balls_53x29_4spp", "c1_random_balls_400x225_10spp_d10"
VIEWS_SCENE = "cornell"  # kernel_classes' name of ragged_cornell_37x37_4spp
SHARD = dict(shard_index=1, shard_count=3)


def handout_frames(rt):
    """What a child renders under its RT_JOBS_PER_GRAB / RT_GRAB_TAPER: {name: array}, and the large frame's launch"""
    import kernel_classes as kc
    import scene_cases
    from job_mode_helpers import VIEWS_SEED, listed, views_on_device
    frames = {}
    for name in DENSE + (LARGE,):
        hs = scene_cases.build(rt, name)
        ds = rt.DeviceScene(hs)
        frames["dense--" + name] = ds.render(rt.render_params(seed=HANDOUT_SEED))
        if name == LARGE:
            launch = rt.debug_last_launch()
        if name == RAGGED:
            frames["tiles--" + name] = ds.render(rt.render_params(seed=HANDOUT_SEED, out_layout=rt.RT_OUT_TILES, **SHARD))
            pixels, _ = kc.stress_list(hs.width * hs.height)
            frames["list--" + name], frames["list_sq--" + name], _ = listed(rt, ds, hs, pixels, [(0, hs.camera.samples_per_pixel)])
        ds.close()
    hs = kc.scene(rt, VIEWS_SCENE)
    ds = rt.DeviceScene(hs)
    frames["views"], frames["guards"] = views_on_device(rt, ds, kc.three_views(rt, VIEWS_SCENE, VIEWS_SEED), kc.spp_of(VIEWS_SCENE))
    ds.close()
    return frames, launch


if __name__ == "__main__":  # the child: python schedule_cases.py OUT.npz
    import importlib
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root), str(root / "tests")]
    rt = importlib.import_module("rust-tracing_amd")
    frames, launch = handout_frames(rt)
    np.savez(sys.argv[1], **frames)
    print(json.dumps({"launch": launch}))
