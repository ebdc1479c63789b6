"""`rtrace --upsample F [--upsample-albedo] [--upsample-edges]`: the PNG has the full size and holds the pixels of the Python chain render
under the scaled camera -> (denoise at the low size) -> upsample -> output stage, with each guide set, behind --denoise and in front of
the tone mapper; the live route's three passes, plain and behind --live-denoise and --live-denoise-albedo, with the guides rendered once;
and what the flags cannot go with ends with status 2 before anything is rendered."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 4
ARGS = ["-s", "6", "--width", str(W), "--aspect", "1.3333333333333333", "--spp", str(SPP), "--depth", "8", "--seed", "5", "--scene-seed", "1"]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path) + ".png").convert("RGB"))


def _rtrace(rt, *args):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    return subprocess.run([str(exe), *ARGS, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def frames(rt):
    """the Cornell box at 64 x 48: the scene, and the full-size guide frames of sums, rendered once"""
    hs = rt.HostScene(6, scene_seed=1, width=W, aspect=4.0 / 3.0, spp=SPP, depth=8)
    assert (hs.width, hs.height) == (W, H)
    p = rt.render_params(seed=5)
    albedo = rt.DeviceScene(hs, device=0, albedo=True).render(p, camera=rt.albedo_camera(hs.camera)).reshape(H, W, 3)
    ids = rt.DeviceScene(hs, device=0, surface_ids=True).render(p, camera=rt.surface_id_camera(hs.camera)).reshape(H, W, 3)
    for a in (albedo, ids):
        a.setflags(write=False)
    return hs, rt.DeviceScene(hs, device=0), albedo, ids


def _guides(flags, albedo, ids):
    kw = {}
    if "--upsample-albedo" in flags:
        kw.update(albedo_sum=albedo, albedo_spp=SPP)
    if "--upsample-edges" in flags:
        kw.update(edge_sum=ids, edge_spp=SPP)
    return kw


@pytest.mark.parametrize("flags", [[], ["--upsample-edges"], ["--upsample-albedo"], ["--upsample-albedo", "--upsample-edges"]], ids=lambda f: "+".join(f) or "tent")
def test_a_plain_render_is_traced_small_and_shown_at_full_size(rt, gpu, frames, tmp_path, flags):
    hs, scene, albedo, ids = frames
    cam = rt.camera_scaled(hs.camera, 2)
    low = scene.render(rt.render_params(seed=5), camera=cam).reshape(cam.image_height, cam.image_width, 3)
    assert low.shape == (24, 32, 3)
    means = rt.upsample(low, SPP, (W, H), factor=2, **_guides(flags, albedo, ids))
    want = np.asarray(rt.resolve_rgb8_host(W, H, 1, means)).reshape(H, W, 3)
    r = _rtrace(rt, "--upsample", "2", *flags, "-o", str(tmp_path / "up"))
    assert r.returncode == 0, r.stderr
    got = _png(tmp_path / "up")
    assert got.shape == (H, W, 3) and np.array_equal(got, want) and len(np.unique(got)) > 8


def test_factor_three_rounds_the_low_size_up(rt, gpu, frames, tmp_path):
    hs, scene, albedo, ids = frames
    cam = rt.camera_scaled(hs.camera, 3)
    assert (cam.image_width, cam.image_height) == (22, 16)
    low = scene.render(rt.render_params(seed=5), camera=cam).reshape(16, 22, 3)
    means = rt.upsample(low, SPP, (W, H), factor=3, albedo_sum=albedo, albedo_spp=SPP, edge_sum=ids, edge_spp=SPP)
    r = _rtrace(rt, "--upsample", "3", "--upsample-albedo", "--upsample-edges", "--tonemap", "aces", "-o", str(tmp_path / "three"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "three"), rt.tonemap(means, 1, op="aces"))


def test_the_denoiser_runs_at_the_low_size_in_front_of_the_upsampler(rt, gpu, frames, tmp_path):
    hs, scene, albedo, ids = frames
    cam = rt.camera_scaled(hs.camera, 2)
    S, Q = scene.render_moments(rt.render_params(seed=5, sample_end=SPP), camera=cam)
    S, Q = S.reshape(24, 32, 3), Q.reshape(24, 32, 3)
    plain = rt.denoise(S, Q, SPP)
    means = rt.upsample(plain, 1, (W, H), factor=2, edge_sum=ids, edge_spp=SPP)
    r = _rtrace(rt, "--denoise", "--upsample", "2", "--upsample-edges", "-o", str(tmp_path / "dn"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "dn"), np.asarray(rt.resolve_rgb8_host(W, H, 1, means)).reshape(H, W, 3))
    # the guided filter takes LOW-size guides, rendered under the scaled camera; bloom and the tone mapper follow on the full-size frame
    p = rt.render_params(seed=5, sample_end=SPP)
    low_albedo = rt.DeviceScene(hs, device=0, albedo=True).render(p, camera=rt.albedo_camera(cam)).reshape(24, 32, 3)
    low_ids = rt.DeviceScene(hs, device=0, surface_ids=True).render(p, camera=rt.surface_id_camera(cam)).reshape(24, 32, 3)
    guided = rt.denoise_guided(S, Q, SPP, low_ids, SPP, albedo_sum=low_albedo, albedo_spp=SPP)
    means = rt.upsample(guided, 1, (W, H), factor=2, albedo_sum=albedo, albedo_spp=SPP, edge_sum=ids, edge_spp=SPP)
    r = _rtrace(rt, "--denoise-albedo", "--denoise-edges", "--upsample", "2", "--upsample-albedo", "--upsample-edges", "--bloom", "--tonemap", "aces",
                "-o", str(tmp_path / "all"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "all"), rt.tonemap(rt.bloom(means, 1), 1, op="aces"))


def test_the_live_route_runs_three_passes_and_shows_the_upsampled_frame(rt, gpu, frames, tmp_path):
    """--spp 4 is three passes of one sample; the guides are rendered once, at min(spp - 1, 16) = 3 samples per pixel, at the full size;
    every pass traces — and filters — the 32 x 24 frame of the scaled camera and shows the 64 x 48 one"""
    hs, scene, _, _ = frames
    cam = rt.camera_scaled(hs.camera, 2)
    p = rt.render_params(seed=5, sample_end=SPP - 1)
    albedo = rt.DeviceScene(hs, device=0, albedo=True).render(p, camera=rt.albedo_camera(hs.camera)).reshape(H, W, 3)
    ids = rt.DeviceScene(hs, device=0, surface_ids=True).render(p, camera=rt.surface_id_camera(hs.camera)).reshape(H, W, 3)
    guides = dict(albedo_sum=albedo, albedo_spp=SPP - 1, edge_sum=ids, edge_spp=SPP - 1)
    flags = ["--upsample", "2", "--upsample-albedo", "--upsample-edges"]
    mean, m2 = scene.render_mean_moments(p, camera=cam)
    assert mean.shape == (24, 32, 3)

    _, want = rt.upsample(mean, 1, (W, H), factor=2, rgba8=True, **guides)
    r = _rtrace(rt, "-l", *flags, "-o", str(tmp_path / "live"))
    assert r.returncode == 0, r.stderr
    assert "Live: 3 frames, 3 samples per pixel in the last" in r.stdout, r.stdout
    got = _png(tmp_path / "live")
    assert got.shape == (H, W, 3) and np.array_equal(got, want[:, :, :3]) and len(np.unique(got)) > 8
    r = _rtrace(rt, "--live", "--live-spp", "2", *flags, "-o", str(tmp_path / "two"))   # passes of two samples end in the same frame
    assert r.returncode == 0 and "Live: 2 frames, 3 samples per pixel in the last" in r.stdout, (r.stdout, r.stderr)
    assert np.array_equal(_png(tmp_path / "two"), got)

    shown = rt.denoise_mean(mean, m2, SPP - 1)                                            # the low frame's own filter, in front
    _, want = rt.upsample(shown, 1, (W, H), factor=2, rgba8=True, **guides)
    r = _rtrace(rt, "-l", "--live-denoise", *flags, "-o", str(tmp_path / "dn"))
    assert r.returncode == 0 and "Live: 3 frames" in r.stdout, (r.stdout, r.stderr)
    assert np.array_equal(_png(tmp_path / "dn"), want[:, :, :3]) and not np.array_equal(want[:, :, :3], got)

    low_albedo = rt.DeviceScene(hs, device=0, albedo=True).render_mean(p, camera=rt.albedo_camera(cam))   # the filter's guide: low size
    shown = rt.denoise_albedo_mean(mean, m2, SPP - 1, low_albedo)
    means = rt.upsample(shown, 1, (W, H), factor=2, **guides)
    r = _rtrace(rt, "-l", "--live-denoise-albedo", *flags, "--tonemap", "aces", "-o", str(tmp_path / "all"))
    assert r.returncode == 0 and "Live: 3 frames" in r.stdout, (r.stdout, r.stderr)
    assert np.array_equal(_png(tmp_path / "all"), rt.tonemap(means, 1, op="aces"))


def test_what_the_flags_cannot_go_with_ends_with_status_2(rt, gpu, tmp_path):
    out = ["-o", str(tmp_path / "never")]
    for flags in (["--upsample", "2", "--orbit", "3"], ["--upsample", "2", "--adaptive", "0.05"], ["--upsample", "2", "--gpus", "2"],
                  ["--upsample", "2", "--progressive", "2"], ["--upsample", "2", "-l", "--gpus", "2"], ["--upsample-albedo"], ["-l", "--upsample-edges"], ["--upsample-edges"],
                  ["--upsample-albedo", "--upsample-edges", "--denoise"], ["--upsample", "1"], ["--upsample", "5"], ["--upsample", "two"]):
        r = _rtrace(rt, *flags, *out)
        assert r.returncode == 2, (flags, r.returncode, r.stderr)
        assert not (tmp_path / "never.png").exists(), flags
