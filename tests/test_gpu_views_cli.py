"""`rtrace --orbit N` (rust-tracing_amd/host/main.cpp): N views around the scene's look_at from one rt_render_views call, one PNG
per view.  View 0 is the plain run's file byte for byte; view 1 is the CPU oracle's frame under camera_look of the turned look_from
at seed + 1, resolved and encoded by the host library."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# Scene 6 (Cornell, black background) is the issue's case; its turned views stand beside and behind the box, where every frame is
# black whatever the camera and seed are.  Scene 0 (random spheres under a sky) is what holds the turn and the seed to the oracle:
# every view of it sees the scene.
@pytest.mark.parametrize("scene, sees_the_scene", [(6, False), (0, True)])
def test_rtrace_orbit_writes_one_png_per_view(rt, oracle, gpu, tmp_path, scene, sees_the_scene):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    args = ["-s", str(scene), "--width", "64", "--spp", "8"]
    plain, orbit = tmp_path / "plain", tmp_path / "X"
    r = subprocess.run([str(exe), *args, "-o", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), *args, "--orbit", "3", "-o", str(orbit)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "3 views" in r.stdout
    files = sorted(p.name for p in tmp_path.glob("X_*.png"))
    assert files == ["X_000.png", "X_001.png", "X_002.png"], files
    assert (tmp_path / "X_000.png").read_bytes() == (tmp_path / "plain.png").read_bytes()

    hs = rt.HostScene(scene, scene_seed=1, width=64, spp=8)  # rtrace's defaults: --scene-seed 1, --seed 1
    # (tests/test_views_host.py holds orbit_look_from to a rotation matrix: the way and the axis of the turn)

    def png(k, seed):
        sums = oracle.render(hs, rt.render_params(seed=seed), camera=rt.camera_look(hs, rt.orbit_look_from(hs, k, 3)))
        path = tmp_path / f"want_{k}_{seed}.png"
        rt.write_png(str(path), rt.resolve_rgb8_host(hs.width, hs.height, 8, sums))
        return sums, path.read_bytes()

    for k in (1, 2):
        sums, want = png(k, 1 + k)
        assert (tmp_path / f"X_{k:03d}.png").read_bytes() == want, f"view {k}"
        if sees_the_scene:
            # the comparison means something: the view is lit all over, another seed or the other view's place give another file
            assert (sums != 0).mean() > 0.9
            assert png(k, 1)[1] != want and png(3 - k, 1 + k)[1] != want
    assert (tmp_path / "X_001.png").read_bytes() != (tmp_path / "X_000.png").read_bytes()


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--progressive", "4"], ["--adaptive", "0.05"]])
def test_rtrace_orbit_refuses_what_it_cannot_be_combined_with(rt, gpu, tmp_path, extra):
    exe = rt.LIB_DIR / "rtrace"
    r = subprocess.run([str(exe), "-s", "6", "--width", "64", "--spp", "8", "--orbit", "3", *extra, "-o", str(tmp_path / "X")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--orbit" in r.stderr and "Usage" in r.stderr, (r.returncode, r.stderr)
    assert not list(tmp_path.glob("*.png"))
