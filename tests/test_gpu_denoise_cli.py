"""`rtrace --denoise`: the PNG is written from the denoised mean — the bytes the Python route (render_moments, then denoise) gives —
with a plain render and with --adaptive; combined with --live it is refused."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_rtrace_denoise_writes_the_python_routes_bytes(rt, gpu, tmp_path):
    from PIL import Image
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    args = ["-s", "6", "--width", "32", "--aspect", "1.0", "--spp", "8", "--depth", "8", "--seed", "5", "--scene-seed", "1"]
    hs = rt.HostScene(6, scene_seed=1, width=32, aspect=1.0, spp=8, depth=8)
    assert (hs.width, hs.height) == (32, 32)
    ds = rt.DeviceScene(hs)
    S, Q = ds.render_moments(rt.render_params(seed=5, sample_end=8))
    _, want = rt.denoise(S, Q, 8, rgba8=True)
    assert len(np.unique(want[:, :, :3])) > 8
    plain = rt.resolve_rgb8_host(32, 32, 8, S)
    assert not np.array_equal(want[:, :, :3], plain), "the denoised frame shows the undenoised bytes"

    out = tmp_path / "dn"
    r = subprocess.run([str(exe), *args, "--denoise", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    a = np.asarray(Image.open(str(out) + ".png").convert("RGB"))
    assert a.shape == (32, 32, 3) and np.array_equal(a, want[:, :, :3])

    # the knobs reach the filter
    _, want2 = rt.denoise(S, Q, 8, rgba8=True, iterations=2, sigma=1.5)
    out2 = tmp_path / "dn2"
    r = subprocess.run([str(exe), *args, "--denoise", "--denoise-iters", "2", "--denoise-sigma", "1.5", "-o", str(out2)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(str(out2) + ".png").convert("RGB")), want2[:, :, :3])
    assert not np.array_equal(want2, want)

    # --adaptive: the adaptive sums, sums of squares and spp map
    S3, spp, Q3, _ = ds.render_adaptive(rt.render_params(seed=5, sample_end=8), min_spp=4, batch_spp=2, rel=0.05)
    _, want3 = rt.denoise(S3, Q3, 0, spp_map=spp, rgba8=True)
    out3 = tmp_path / "dn3"
    r = subprocess.run([str(exe), *args, "--denoise", "--adaptive", "0.05", "--min-spp", "4", "--batch-spp", "2", "-o", str(out3)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(str(out3) + ".png").convert("RGB")), want3[:, :, :3])


def test_rtrace_refuses_denoise_with_live_and_with_several_gpus(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "-o", str(tmp_path / "x"), "--denoise"]
    for extra in (["--live"], ["-l"], ["--gpus", "2"]):
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, (extra, r.stdout)
        assert "--denoise" in r.stderr and "--live" in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    for args in ([*base[:-1], "--denoise-iters", "3"], [*base, "--denoise-iters", "7"], [*base, "--denoise-sigma", "0"]):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--denoise" in r.stderr, (args, r.stderr)
    assert not list(tmp_path.iterdir())
