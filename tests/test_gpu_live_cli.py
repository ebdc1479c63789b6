"""`rtrace -l/--live`: the reference's live mode without the window.  It folds spp - 1 samples into a running mean (the reference's loop
draws only while num_samples < spp, src/renderer.rs:104) and writes the last frame's RGB bytes to OUTPUT.png; the expected pixels are
color_to_rgb of the recurrence over the CPU oracle's single-sample frames."""
import subprocess

import numpy as np
import pytest

import live_helpers

pytestmark = pytest.mark.gpu


def test_rtrace_live_writes_the_running_mean_of_spp_minus_one_samples(rt, oracle, gpu, tmp_path):
    from PIL import Image
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    args = ["-s", "6", "--width", "24", "--aspect", "1.5", "--spp", "5", "--depth", "8", "--seed", "5", "--scene-seed", "1"]
    hs = rt.HostScene(6, scene_seed=1, width=24, aspect=1.5, spp=5, depth=8)
    assert (hs.width, hs.height) == (24, 16)
    colours = live_helpers.oracle_samples(rt, oracle, hs, 5, 5)
    mean4, mean5 = live_helpers.fold(colours[:4]), live_helpers.fold(colours)
    want = rt.resolve_rgb8_host(24, 16, 1, mean4)
    assert not np.array_equal(want, rt.resolve_rgb8_host(24, 16, 1, mean5)), "four and five samples show the same frame"
    assert len(np.unique(want)) > 8

    one = tmp_path / "one"
    r = subprocess.run([str(exe), *args, "--live", "-o", str(one)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Args: { live: true" in r.stdout and "Live: 4 frames, 4 samples per pixel in the last" in r.stdout, r.stdout
    a = np.asarray(Image.open(str(one) + ".png").convert("RGB"))
    assert a.shape == (16, 24, 3) and np.array_equal(a, want)

    two = tmp_path / "two"
    r = subprocess.run([str(exe), *args, "-l", "--live-spp", "2", "-o", str(two)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Live: 2 frames, 4 samples per pixel in the last" in r.stdout, r.stdout
    assert (tmp_path / "two.png").read_bytes() == (tmp_path / "one.png").read_bytes()
