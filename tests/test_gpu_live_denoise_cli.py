"""`rtrace -l --live-denoise` and `--live-denoise-albedo`: the last frame's PNG holds the bytes the Python route gives for the same scene,
seed and spp - 1 samples (render_mean_moments, the albedo scene's render_mean under the white-background camera, then denoise_mean /
denoise_albedo_mean); the flags need --live, and a knob needs its flag."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path) + ".png").convert("RGB"))


def test_rtrace_live_denoise_writes_the_python_routes_bytes(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    args = ["-s", "6", "--width", "37", "--aspect", "1.0", "--spp", "6", "--depth", "8", "--seed", "5", "--scene-seed", "1"]
    hs = rt.HostScene(6, scene_seed=1, width=37, aspect=1.0, spp=6, depth=8)  # the ragged Cornell case
    assert (hs.width, hs.height) == (37, 37)
    mean, m2, unfiltered = rt.DeviceScene(hs).render_mean_moments(rt.render_params(seed=5, sample_end=5), rgba8=True)   # spp - 1 samples
    _, want = rt.denoise_mean(mean, m2, 5, rgba8=True)
    assert len(np.unique(want[:, :, :3])) > 8 and not np.array_equal(want, unfiltered), "the filtered frame shows the mean's bytes"

    one = tmp_path / "one"
    r = subprocess.run([str(exe), *args, "-l", "--live-denoise", "-o", str(one)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Live: 5 frames, 5 samples per pixel in the last" in r.stdout, r.stdout
    a = png(one)
    assert a.shape == (37, 37, 3) and np.array_equal(a, want[:, :, :3])
    # passes of two samples end in the same frame: the filter never writes the running mean or M2
    two = tmp_path / "two"
    r = subprocess.run([str(exe), *args, "--live", "--live-spp", "2", "--live-denoise", "-o", str(two)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Live: 3 frames, 5 samples per pixel in the last" in r.stdout, r.stdout
    assert np.array_equal(png(two), a)
    # the knobs reach the filter
    _, want3 = rt.denoise_mean(mean, m2, 5, rgba8=True, iterations=2, sigma=1.5)
    three = tmp_path / "three"
    r = subprocess.run([str(exe), *args, "-l", "--live-denoise", "--denoise-iters", "2", "--denoise-sigma", "1.5", "-o", str(three)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(three), want3[:, :, :3]) and not np.array_equal(want3, want)
    # the plain live route is what it was
    plain = tmp_path / "plain"
    r = subprocess.run([str(exe), *args, "-l", "-o", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(plain), unfiltered[:, :, :3])


def test_rtrace_live_denoise_albedo_writes_the_python_routes_bytes_on_a_textured_scene(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    args = ["-s", "1", "--width", "40", "--aspect", "1.6", "--spp", "5", "--depth", "8", "--seed", "3", "--scene-seed", "1"]
    hs = rt.HostScene(1, scene_seed=1, width=40, aspect=1.6, spp=5, depth=8)  # two checkered spheres
    assert (hs.width, hs.height) == (40, 25)
    p = rt.render_params(seed=3, sample_end=4)
    mean, m2 = rt.DeviceScene(hs).render_mean_moments(p)
    albedo = rt.DeviceScene(hs, albedo=True).render_mean(p, camera=rt.albedo_camera(hs.camera))
    _, want = rt.denoise_albedo_mean(mean, m2, 4, albedo, rgba8=True)
    _, plain = rt.denoise_mean(mean, m2, 4, rgba8=True)
    assert len(np.unique(want[:, :, :3])) > 8 and not np.array_equal(want, plain), "the guided frame shows the plain filter's bytes"

    out = tmp_path / "g"
    r = subprocess.run([str(exe), *args, "-l", "--live-denoise-albedo", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Live: 4 frames, 4 samples per pixel in the last" in r.stdout, r.stdout
    a = png(out)
    assert a.shape == (25, 40, 3) and np.array_equal(a, want[:, :, :3])
    _, want2 = rt.denoise_albedo_mean(mean, m2, 4, albedo, rgba8=True, iterations=2, sigma=1.5, sigma_albedo=0.1)
    out2 = tmp_path / "g2"
    r = subprocess.run([str(exe), *args, "--live", "--live-spp", "3", "--live-denoise-albedo", "--denoise-albedo-sigma", "0.1", "--denoise-iters", "2",
                        "--denoise-sigma", "1.5", "-o", str(out2)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(out2), want2[:, :, :3]) and not np.array_equal(want2, want)


def test_rtrace_refuses_the_new_flags_without_live_and_a_knob_without_its_flag(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "-o", str(tmp_path / "x")]
    for extra, word in ((["--live-denoise"], "--live"), (["--live-denoise-albedo"], "--live"),
                        (["--live-denoise-albedo", "--denoise-albedo-sigma", "0.2"], "--live"),
                        (["--live", "--denoise-iters", "3"], "--live-denoise"), (["--live", "--denoise-sigma", "2"], "--live-denoise"),
                        (["--live", "--live-denoise", "--denoise-albedo-sigma", "0.3"], "--live-denoise-albedo"),
                        (["--live", "--live-denoise", "--denoise"], "--denoise"), (["--live", "--live-denoise-albedo", "--denoise-albedo"], "--denoise")):
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (extra, r.stderr)
    assert not list(tmp_path.iterdir())
