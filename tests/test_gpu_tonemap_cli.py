"""`rtrace --tonemap / --exposure / --auto-exposure / --tonemap-white`: the PNG holds the bytes the stage's host mirror gives for the
route's own sums (plain) or running mean (-l), `--tonemap clamp` alone changes nothing, and what the flags cannot be combined with ends
with status 2 before anything is rendered."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGS = ["-s", "6", "--width", "24", "--aspect", "1.5", "--spp", "5", "--depth", "8", "--seed", "5", "--scene-seed", "1"]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path) + ".png").convert("RGB"))


def _rtrace(rt, *args):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    return subprocess.run([str(exe), *ARGS, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def scene(rt):
    hs = rt.HostScene(6, scene_seed=1, width=24, aspect=1.5, spp=5, depth=8)
    assert (hs.width, hs.height) == (24, 16)
    return hs, rt.DeviceScene(hs, device=0)


def test_a_plain_render_is_written_through_the_stage(rt, gpu, scene, tmp_path):
    hs, ds = scene
    sums = ds.render(rt.render_params(seed=5)).reshape(16, 24, 3)
    want = rt.tonemap_host(sums, 5, op="aces", exposure=0.5)
    assert not np.array_equal(want, rt.resolve_rgb8_host(24, 16, 5, sums)) and len(np.unique(want)) > 8
    r = _rtrace(rt, "--tonemap", "aces", "--exposure", "-1", "-o", str(tmp_path / "aces"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "aces"), want)
    # Reinhard with a white point, exposed by the frame's own log-average
    want = rt.tonemap_host(sums, 5, op="reinhard", white=2.0, auto_key=0.18)
    r = _rtrace(rt, "--tonemap", "reinhard", "--tonemap-white", "2", "--auto-exposure", "-o", str(tmp_path / "reinhard"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "reinhard"), want)


def test_the_clamp_alone_writes_what_no_flag_writes(rt, gpu, tmp_path):
    r = _rtrace(rt, "-o", str(tmp_path / "none"))
    assert r.returncode == 0, r.stderr
    r2 = _rtrace(rt, "--tonemap", "clamp", "-o", str(tmp_path / "clamp"))
    assert r2.returncode == 0, r2.stderr
    assert (tmp_path / "clamp.png").read_bytes() == (tmp_path / "none.png").read_bytes()
    # and on the routes that end on the device: the adaptive one's map, the filter's means
    for flags in (["--adaptive", "0.05", "--min-spp", "2", "--batch-spp", "2"], ["--denoise"]):
        a = _rtrace(rt, *flags, "-o", str(tmp_path / "a"))
        b = _rtrace(rt, *flags, "--tonemap", "clamp", "-o", str(tmp_path / "b"))
        assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
        assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes(), flags


def test_a_live_frame_is_exposed_by_its_own_log_average(rt, gpu, scene, tmp_path):
    hs, ds = scene
    mean = ds.render_mean(rt.render_params(seed=5, sample_end=4))   # --live settles on spp - 1 samples
    want = rt.tonemap_host(mean, 1, auto_key=0.18)
    assert not np.array_equal(want, rt.resolve_rgb8_host(24, 16, 1, mean))
    r = _rtrace(rt, "-l", "--auto-exposure", "-o", str(tmp_path / "live"))
    assert r.returncode == 0, r.stderr
    assert "Live: 4 frames, 4 samples per pixel in the last" in r.stdout, r.stdout
    assert np.array_equal(_png(tmp_path / "live"), want)
    want = rt.tonemap_host(mean, 1, op="aces", auto_key=0.5)
    r = _rtrace(rt, "-l", "--live-spp", "2", "--tonemap", "aces", "--auto-exposure", "0.5", "-o", str(tmp_path / "live2"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "live2"), want)


def test_what_the_flags_cannot_go_with_ends_with_status_2(rt, gpu, tmp_path):
    out = ["-o", str(tmp_path / "never")]
    for flags in (["--tonemap", "aces", "--gpus", "2"], ["--exposure", "1", "--gpus", "2"], ["--auto-exposure", "--progressive", "2"],
                  ["--tonemap", "reinhard", "--progressive", "2"], ["--tonemap-white", "4"], ["--tonemap-white", "4", "--tonemap", "aces"],
                  ["--tonemap", "filmic"], ["--exposure", "65"], ["--exposure", "nan"], ["--exposure", "two"], ["--auto-exposure", "0"],
                  ["--tonemap-white", "0", "--tonemap", "reinhard"]):
        r = _rtrace(rt, *flags, *out)
        assert r.returncode == 2, (flags, r.returncode, r.stderr)
        assert not (tmp_path / "never.png").exists(), flags
