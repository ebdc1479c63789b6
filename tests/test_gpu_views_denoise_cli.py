"""`rtrace --orbit N --orbit-denoise` and `--orbit-denoise-albedo`: one PNG per view, written from that view's filtered mean — the
bytes the Python route gives (render_views_moments, for the guided form render_views of the albedo scene under the views' cameras with
a white background, then denoise_views / denoise_albedo_views) — and the refusals of the two flags."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SPP, SEED = 3, 8, 5


def python_route(rt, scene, guided, **kw):
    hs = rt.HostScene(scene, scene_seed=1, width=64, spp=SPP, depth=8)
    assert hs.width == 64
    views = rt.orbit_views(hs, N, SEED)
    p = rt.render_params(sample_end=SPP)
    S, Q = rt.DeviceScene(hs).render_views_moments(p, views)
    if not guided:
        return hs, S, Q, rt.denoise_views(S, Q, SPP, rgba8=True, **kw)[1]
    white = rt.orbit_views(hs, N, SEED)
    for k in range(N):
        white[k].camera = rt.albedo_camera(views[k].camera)
    A = rt.DeviceScene(hs, albedo=True).render_views(p, white)
    return hs, S, Q, rt.denoise_albedo_views(S, Q, SPP, A, SPP, rgba8=True, **kw)[1]


def run_rtrace(rt, scene, out, *flags):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    args = ["-s", str(scene), "--width", "64", "--spp", str(SPP), "--depth", "8", "--seed", str(SEED), "--scene-seed", "1", "--orbit", str(N)]
    return subprocess.run([str(exe), *args, *flags, "-o", str(out)], capture_output=True, text=True, timeout=300)


def pngs(out, hs):
    from PIL import Image
    frames = [np.asarray(Image.open(f"{out}_{k:03d}.png").convert("RGB")) for k in range(N)]
    assert all(f.shape == (hs.height, hs.width, 3) for f in frames)
    return frames


def test_rtrace_orbit_denoise_writes_the_python_routes_bytes_per_view(rt, gpu, tmp_path):
    hs, S, Q, want = python_route(rt, 0, False)  # random balls
    r = run_rtrace(rt, 0, tmp_path / "od", "--orbit-denoise")
    assert r.returncode == 0, r.stderr
    got = pngs(tmp_path / "od", hs)
    assert sorted(f.name for f in tmp_path.iterdir()) == [f"od_{k:03d}.png" for k in range(N)]
    unfiltered = rt.resolve_rgb8_host(hs.width, hs.height, SPP, S[0])
    for k in range(N):
        assert np.array_equal(got[k], want[k][:, :, :3]), f"view {k}"
    assert not np.array_equal(got[0], unfiltered), "the PNG shows the unfiltered frame"
    assert len({f.tobytes() for f in got}) == N
    # the knobs reach the filter
    want2 = python_route(rt, 0, False, iterations=2, sigma=1.5)[3]
    r = run_rtrace(rt, 0, tmp_path / "od2", "--orbit-denoise", "--denoise-iters", "2", "--denoise-sigma", "1.5")
    assert r.returncode == 0, r.stderr
    got2 = pngs(tmp_path / "od2", hs)
    for k in range(N):
        assert np.array_equal(got2[k], want2[k][:, :, :3]), f"view {k}, K = 2, sigma = 1.5"
    assert not np.array_equal(want2, want)


def test_rtrace_orbit_denoise_albedo_writes_the_python_routes_bytes_per_view(rt, gpu, tmp_path):
    hs, S, Q, want = python_route(rt, 3, True, sigma_albedo=0.3)  # two perlin spheres: textured
    plain = rt.denoise_views(S, Q, SPP, rgba8=True)[1]
    assert not np.array_equal(want, plain), "the guide changed nothing on a textured scene"
    r = run_rtrace(rt, 3, tmp_path / "oa", "--orbit-denoise-albedo", "--denoise-albedo-sigma", "0.3")
    assert r.returncode == 0, r.stderr
    got = pngs(tmp_path / "oa", hs)
    assert sorted(f.name for f in tmp_path.iterdir()) == [f"oa_{k:03d}.png" for k in range(N)]
    for k in range(N):
        assert np.array_equal(got[k], want[k][:, :, :3]), f"view {k}"


def test_rtrace_refuses_the_orbit_filters_where_they_do_not_apply(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "-o", str(tmp_path / "x")]
    cases = [
        (["--orbit-denoise"], "--orbit"),                                           # either flag without --orbit
        (["--orbit-denoise-albedo"], "--orbit"),
        (["--orbit", "3", "--orbit-denoise", "--orbit-denoise-albedo"], "--orbit-denoise"),   # both together
        (["--orbit", "3", "--denoise"], "--denoise"),                               # as before: --denoise does not take --orbit
        (["--orbit", "3", "--denoise-albedo"], "--denoise"),
        (["--orbit", "3", "--denoise-iters", "2"], "--denoise"),                    # a knob without any denoise flag
        (["--orbit", "3", "--denoise-sigma", "2"], "--denoise"),
        (["--orbit", "3", "--denoise-albedo-sigma", "0.3"], "--denoise-albedo"),
        (["--orbit", "3", "--orbit-denoise", "--denoise-albedo-sigma", "0.3"], "--denoise-albedo"),   # the guided knob with the plain filter
        (["--orbit", "3", "--orbit-denoise", "--denoise-iters", "9"], "--denoise-iters"),
        (["--orbit", "3", "--orbit-denoise", "--gpus", "2"], "--orbit"),            # --orbit's own exclusions stand
        (["--live", "--orbit-denoise"], "--orbit"),
    ]
    for extra, word in cases:
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert word in r.stderr, (extra, r.stderr)
    assert not list(tmp_path.iterdir())
