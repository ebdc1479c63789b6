"""`rtrace -l --live-denoise-edges` and `rtrace --orbit N --orbit-denoise-edges`: the PNGs hold the bytes the same pipelines give when
driven through the Python bindings — the live route's running mean and M2 after every pass, the surface-ID scene's frame of means
rendered once (min(spp - 1, 16) samples, black background, the session's seed), denoise_guided_mean[_spatial] on the last pass; the
orbit's moments from one views launch, the surface-ID views from another, denoise_guided_views over the stack — and the flags' refusals."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, SEED = 48, 9


def png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def run_rtrace(rt, out, *flags):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    args = ["-s", "6", "--width", str(W), "--aspect", "1", "--depth", "8", "--seed", str(SEED), "--scene-seed", "1"]
    return subprocess.run([str(exe), *args, *flags, "-o", str(out)], capture_output=True, text=True, timeout=300)


def live_python_route(rt, spp, albedo, spatial, **kw):
    """the last frame of `rtrace -l --live-spp 1 --spp spp --live-denoise-edges ...`: (rgb bytes, the unguided filter's rgb bytes)"""
    hs = rt.HostScene(6, scene_seed=1, width=W, aspect=1.0, spp=spp, depth=8)  # the Cornell box
    last = spp - 1
    p = rt.render_params(seed=SEED, sample_end=last)
    mean, m2 = rt.DeviceScene(hs).render_mean_moments(p)[:2]
    guide_spp = min(last, 16)
    ids = rt.DeviceScene(hs, surface_ids=True).render_mean(rt.render_params(seed=SEED, sample_end=guide_spp), camera=rt.surface_id_camera(hs.camera))
    ids = ids[0] if isinstance(ids, tuple) else ids
    A = None
    if albedo:
        A = rt.DeviceScene(hs, albedo=True).render_mean(p, camera=rt.albedo_camera(hs.camera))
        A = A[0] if isinstance(A, tuple) else A
    if spatial:
        got = rt.denoise_guided_mean_spatial(mean, m2, last, ids, albedo_mean=A, rgba8=True, spatial_below=2, **kw)[1]
        plain = (rt.denoise_mean_spatial(mean, m2, last, rgba8=True, spatial_below=2) if A is None
                 else rt.denoise_albedo_mean_spatial(mean, m2, last, A, rgba8=True, spatial_below=2))[1]
    else:
        got = rt.denoise_guided_mean(mean, m2, last, ids, albedo_mean=A, rgba8=True, **kw)[1]
        plain = (rt.denoise_mean(mean, m2, last, rgba8=True) if A is None else rt.denoise_albedo_mean(mean, m2, last, A, rgba8=True))[1]
    return hs, got[:, :, :3], plain[:, :, :3]


@pytest.mark.parametrize("spp, flags", [
    (2, ["--live-denoise-spatial"]),                                   # one sample per pixel: the edge-aware spatial prepare
    (2, ["--live-denoise-albedo", "--live-denoise-spatial"]),
    (4, []),                                                           # three samples: the means form
    (4, ["--live-denoise-albedo", "--denoise-edges-sigma", "0.75"]),
])
def test_rtrace_live_denoise_edges_writes_the_python_routes_bytes(rt, gpu, tmp_path, spp, flags):
    kw = dict(sigma_edge=0.75) if "--denoise-edges-sigma" in flags else {}
    hs, want, plain = live_python_route(rt, spp, "--live-denoise-albedo" in flags, "--live-denoise-spatial" in flags, **kw)
    r = run_rtrace(rt, tmp_path / "live", "-l", "--live-spp", "1", "--spp", str(spp), "--live-denoise-edges", *flags)
    assert r.returncode == 0, r.stderr
    got = png(tmp_path / "live.png")
    assert got.shape == (hs.height, hs.width, 3)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, plain), "the edge guide changed nothing on the Cornell box"


@pytest.mark.parametrize("flags", [[], ["--orbit-denoise"], ["--orbit-denoise-albedo"]])
def test_rtrace_orbit_denoise_edges_writes_the_python_routes_bytes_per_view(rt, gpu, tmp_path, flags):
    n, spp = 3, 4
    hs = rt.HostScene(6, scene_seed=1, width=W, aspect=1.0, spp=spp, depth=8)
    views = rt.orbit_views(hs, n, SEED)
    p = rt.render_params(sample_end=spp)
    S, Q = rt.DeviceScene(hs).render_views_moments(p, views)
    black, white = rt.orbit_views(hs, n, SEED), rt.orbit_views(hs, n, SEED)
    for k in range(n):
        black[k].camera = rt.surface_id_camera(views[k].camera)
        white[k].camera = rt.albedo_camera(views[k].camera)
    E = rt.DeviceScene(hs, surface_ids=True).render_views(p, black)
    A = rt.DeviceScene(hs, albedo=True).render_views(p, white) if "--orbit-denoise-albedo" in flags else None
    want = rt.denoise_guided_views(S, Q, spp, E, spp, albedo_sum=A, albedo_spp=spp, rgba8=True)[1]
    r = run_rtrace(rt, tmp_path / "oe", "--spp", str(spp), "--orbit", str(n), "--orbit-denoise-edges", *flags)
    assert r.returncode == 0, r.stderr
    assert sorted(f.name for f in tmp_path.iterdir()) == [f"oe_{k:03d}.png" for k in range(n)]
    for k in range(n):
        assert np.array_equal(png(tmp_path / f"oe_{k:03d}.png"), want[k][:, :, :3]), f"view {k}"
    plain = (rt.denoise_views(S, Q, spp, rgba8=True) if A is None else rt.denoise_albedo_views(S, Q, spp, A, spp, rgba8=True))[1]
    assert not np.array_equal(want, plain), "the edge guide changed nothing"


def test_rtrace_refuses_the_new_flags_where_they_do_not_apply(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "-o", str(tmp_path / "x")]
    cases = [
        (["--live-denoise-edges"], "--live"),                                           # without -l
        (["-l", "--live-denoise-edges", "--upsample", "2"], "--upsample"),              # out of scope: the guide at the low size
        (["-l", "--live-denoise-edges", "--upsample", "2", "--upsample-edges"], "--upsample"),
        (["--orbit-denoise-edges"], "--orbit"),                                         # without --orbit
        (["-l", "--orbit-denoise-edges"], "--orbit"),
        (["-l", "--live-denoise", "--denoise-edges-sigma", "0.3"], "--denoise-edges"),  # the knob still needs one of the three flags
        (["--orbit", "3", "--orbit-denoise", "--denoise-edges-sigma", "0.3"], "--denoise-edges"),
        (["--denoise-edges-sigma", "0.3"], "--denoise-edges"),
        (["-l", "--live-denoise-edges", "--denoise-edges-sigma", "0"], "--denoise-edges-sigma"),
        (["-l", "--denoise-edges"], "--denoise"),                                       # as before: --denoise-edges is not a live flag
        (["-l", "--live-denoise-edges", "--denoise-edges"], "--denoise"),
        (["--orbit", "3", "--denoise-edges"], "--denoise"),
        (["--orbit", "3", "--orbit-denoise-edges", "--orbit-denoise", "--orbit-denoise-albedo"], "--orbit-denoise"),
        (["-l", "--live-denoise-edges", "--gpus", "2"], "--live"),
    ]
    for extra, word in cases:
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert word in r.stderr, (extra, r.stderr)
    assert not list(tmp_path.iterdir())
