"""`rtrace --bloom [STRENGTH] [--bloom-threshold T] [--bloom-levels K]`: the PNG holds the pixels of the Python chain render -> bloom ->
tonemap on a plain render (the host mirror's route) and on --denoise (a device route), and what the flags cannot go with ends with
status 2 before anything is rendered."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGS = ["-s", "5", "--width", "32", "--aspect", "1.3333333333333333", "--spp", "4", "--depth", "8", "--seed", "5", "--scene-seed", "1"]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path) + ".png").convert("RGB"))


def _rtrace(rt, *args):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    return subprocess.run([str(exe), *ARGS, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def scene(rt):
    hs = rt.HostScene(5, scene_seed=1, width=32, aspect=4.0 / 3.0, spp=4, depth=8)   # simple_light
    assert (hs.width, hs.height) == (32, 24)
    return rt.DeviceScene(hs, device=0)


def test_a_plain_render_is_bloomed_in_front_of_the_curve(rt, gpu, scene, tmp_path):
    sums = scene.render(rt.render_params(seed=5)).reshape(24, 32, 3)
    bloomed = rt.bloom(sums, 4)
    want = rt.tonemap(bloomed, 1, op="aces")
    assert not np.array_equal(want, rt.tonemap(sums, 4, op="aces")) and len(np.unique(want)) > 8, "the frame must glow"
    r = _rtrace(rt, "--bloom", "--tonemap", "aces", "-o", str(tmp_path / "aces"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "aces"), want)
    # the knobs reach the call, bloom alone implies the clamp, and auto-exposure sees the bloomed frame
    bloomed = rt.bloom(sums, 4, strength=0.6, threshold=0.5, levels=3)
    r = _rtrace(rt, "--bloom", "0.6", "--bloom-threshold", "0.5", "--bloom-levels", "3", "-o", str(tmp_path / "clamp"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "clamp"), rt.tonemap(bloomed, 1))
    r = _rtrace(rt, "--bloom", "0.6", "--bloom-threshold", "0.5", "--bloom-levels", "3", "--auto-exposure", "-o", str(tmp_path / "auto"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "auto"), rt.tonemap(bloomed, 1, auto_key=0.18))


def test_a_device_route_is_bloomed_on_the_device(rt, gpu, scene, tmp_path):
    S, Q = scene.render_moments(rt.render_params(seed=5, sample_end=4))
    mean, _ = rt.denoise(S, Q, 4, rgba8=True)
    want = rt.tonemap(rt.bloom(mean, 1), 1, op="aces")
    assert not np.array_equal(want, rt.tonemap(mean, 1, op="aces"))
    r = _rtrace(rt, "--denoise", "--bloom", "--tonemap", "aces", "-o", str(tmp_path / "dn"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "dn"), want)


def test_what_the_flags_cannot_go_with_ends_with_status_2(rt, gpu, tmp_path):
    out = ["-o", str(tmp_path / "never")]
    for flags in (["--bloom", "--gpus", "2"], ["--bloom", "0.5", "--tonemap", "aces", "--gpus", "2"], ["--bloom", "--progressive", "2"],
                  ["--bloom-threshold", "2"], ["--bloom-levels", "3"], ["--bloom-levels", "3", "--tonemap", "aces"],
                  ["--bloom", "--bloom-levels", "9"], ["--bloom", "--bloom-levels", "0"], ["--bloom", "--bloom-threshold", "-1"],
                  ["--bloom", "--bloom-threshold", "nan"]):
        r = _rtrace(rt, *flags, *out)
        assert r.returncode == 2, (flags, r.returncode, r.stderr)
        assert not (tmp_path / "never.png").exists(), flags
