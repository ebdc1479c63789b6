"""`rtrace -l --live-denoise --live-denoise-spatial` and its albedo form: the first frame — at --spp 2 the only one, of one sample — holds
the bytes the Python route gives (render_mean_moments over one sample, the albedo scene's render_mean under the white-background camera,
then denoise_mean_spatial / denoise_albedo_mean_spatial); later frames are those of --live-denoise alone at the default threshold; the
flags need their flags."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path) + ".png").convert("RGB"))


def run(exe, args, out):
    r = subprocess.run([str(exe), *args, "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout, png(out)


def test_rtrace_shows_the_first_frame_filtered_with_the_python_routes_bytes(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    scene = ["-s", "6", "--width", "37", "--aspect", "1.0", "--depth", "8", "--seed", "5", "--scene-seed", "1"]
    hs = rt.HostScene(6, scene_seed=1, width=37, aspect=1.0, spp=2, depth=8)  # the ragged Cornell case
    assert (hs.width, hs.height) == (37, 37)
    ds = rt.DeviceScene(hs)
    mean, m2, unfiltered = ds.render_mean_moments(rt.render_params(seed=5, sample_end=1), rgba8=True)   # spp - 1 = 1 sample
    _, want = rt.denoise_mean_spatial(mean, None, 1, rgba8=True)
    assert len(np.unique(want[:, :, :3])) > 8 and not np.array_equal(want, unfiltered), "the filtered frame shows the mean's bytes"
    first = [*scene, "--spp", "2", "-l", "--live-denoise"]
    out, a = run(exe, [*first, "--live-denoise-spatial"], tmp_path / "a")
    assert "Live: 1 frames, 1 samples per pixel in the last" in out, out
    assert a.shape == (37, 37, 3) and np.array_equal(a, want[:, :, :3])
    # without the flag the first frame is the unfiltered mean, as it was
    _, b = run(exe, first, tmp_path / "b")
    assert np.array_equal(b, unfiltered[:, :, :3])
    # the radius and the filter's knobs reach the call; N = 1 never takes the spatial route
    _, want3 = rt.denoise_mean_spatial(mean, None, 1, rgba8=True, window_radius=3, iterations=2, sigma=1.5)
    _, c = run(exe, [*first, "--live-denoise-spatial", "2", "--denoise-spatial-radius", "3", "--denoise-iters", "2", "--denoise-sigma", "1.5"], tmp_path / "c")
    assert np.array_equal(c, want3[:, :, :3]) and not np.array_equal(want3, want)
    _, d = run(exe, [*first, "--live-denoise-spatial", "1"], tmp_path / "d")
    assert np.array_equal(d, unfiltered[:, :, :3])
    # later frames: at the default threshold they are --live-denoise's; a higher threshold keeps the spatial route on
    later = [*scene, "--spp", "4", "-l", "--live-denoise"]
    out, e = run(exe, [*later, "--live-denoise-spatial"], tmp_path / "e")
    assert "Live: 3 frames, 3 samples per pixel in the last" in out, out
    _, f = run(exe, later, tmp_path / "f")
    assert np.array_equal(e, f)
    mean3, m23 = ds.render_mean_moments(rt.render_params(seed=5, sample_end=3))
    _, want_m2 = rt.denoise_mean(mean3, m23, 3, rgba8=True)
    assert np.array_equal(f, want_m2[:, :, :3])
    _, want4 = rt.denoise_mean_spatial(mean3, None, 3, rgba8=True, spatial_below=4)
    _, g = run(exe, [*later, "--live-denoise-spatial", "4"], tmp_path / "g")
    assert np.array_equal(g, want4[:, :, :3]) and not np.array_equal(g, f)


def test_rtrace_albedo_form_writes_the_python_routes_bytes_on_a_textured_scene(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    scene = ["-s", "1", "--width", "40", "--aspect", "1.6", "--depth", "8", "--seed", "3", "--scene-seed", "1"]
    hs = rt.HostScene(1, scene_seed=1, width=40, aspect=1.6, spp=2, depth=8)  # two checkered spheres
    assert (hs.width, hs.height) == (40, 25)
    p = rt.render_params(seed=3, sample_end=1)
    mean, m2 = rt.DeviceScene(hs).render_mean_moments(p)
    albedo = rt.DeviceScene(hs, albedo=True).render_mean(p, camera=rt.albedo_camera(hs.camera))
    _, want = rt.denoise_albedo_mean_spatial(mean, None, 1, albedo, rgba8=True)
    _, plain = rt.denoise_mean_spatial(mean, None, 1, rgba8=True)
    assert len(np.unique(want[:, :, :3])) > 8 and not np.array_equal(want, plain), "the guided frame shows the plain route's bytes"
    out, a = run(exe, [*scene, "--spp", "2", "-l", "--live-denoise-albedo", "--live-denoise-spatial"], tmp_path / "a")
    assert "Live: 1 frames, 1 samples per pixel in the last" in out, out
    assert a.shape == (25, 40, 3) and np.array_equal(a, want[:, :, :3])
    _, want2 = rt.denoise_albedo_mean_spatial(mean, None, 1, albedo, rgba8=True, window_radius=2, sigma_albedo=0.1)
    _, b = run(exe, [*scene, "--spp", "2", "--live", "--live-denoise-albedo", "--live-denoise-spatial", "--denoise-spatial-radius", "2",
                     "--denoise-albedo-sigma", "0.1"], tmp_path / "b")
    assert np.array_equal(b, want2[:, :, :3]) and not np.array_equal(want2, want)
    # later frames at the default threshold are --live-denoise-albedo's
    later = [*scene, "--spp", "4", "-l", "--live-denoise-albedo"]
    _, c = run(exe, [*later, "--live-denoise-spatial"], tmp_path / "c")
    _, d = run(exe, later, tmp_path / "d")
    assert np.array_equal(c, d)


def test_rtrace_refuses_the_spatial_flags_without_their_flags(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "-o", str(tmp_path / "x")]
    for extra, word in ((["--live", "--live-denoise-spatial"], "--live-denoise"), (["--live", "--live-denoise-spatial", "3"], "--live-denoise"),
                        (["--live", "--live-denoise", "--denoise-spatial-radius", "2"], "--live-denoise-spatial"),
                        (["--live", "--live-denoise-albedo", "--denoise-spatial-radius", "1"], "--live-denoise-spatial"),
                        (["--live-denoise", "--live-denoise-spatial"], "--live"),
                        (["--live", "--live-denoise", "--live-denoise-spatial", "--denoise"], "--denoise")):
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (extra, r.stderr)
    for extra in (["--live", "--live-denoise", "--live-denoise-spatial", "0"], ["--live", "--live-denoise", "--live-denoise-spatial", "--denoise-spatial-radius", "4"]):
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "spatial" in r.stderr, (extra, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())
