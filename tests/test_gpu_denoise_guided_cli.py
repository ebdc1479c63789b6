"""`rtrace --denoise-edges`: the PNG is written from the edge-guided mean — the bytes the Python route (render_moments, the
surface-ID scene's render under the black-background camera, then denoise_guided) gives; it implies --denoise, may stand beside
--denoise-albedo, and has --denoise's exclusions."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_rtrace_denoise_edges_writes_the_python_routes_bytes(rt, gpu, tmp_path):
    from PIL import Image
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    args = ["-s", "6", "--width", "37", "--aspect", "1.0", "--spp", "4", "--depth", "8", "--seed", "5", "--scene-seed", "1"]
    hs = rt.HostScene(6, scene_seed=1, width=37, aspect=1.0, spp=4, depth=8)  # the ragged Cornell case
    assert (hs.width, hs.height) == (37, 37)
    p = rt.render_params(seed=5, sample_end=4)
    S, Q = rt.DeviceScene(hs).render_moments(p)
    E = rt.DeviceScene(hs, surface_ids=True).render(p, camera=rt.surface_id_camera(hs.camera)).reshape(S.shape)
    A = rt.DeviceScene(hs, albedo=True).render(p, camera=rt.albedo_camera(hs.camera)).reshape(S.shape)
    _, want = rt.denoise_guided(S, Q, 4, E, 4, rgba8=True)
    _, plain = rt.denoise(S, Q, 4, rgba8=True)
    assert len(np.unique(want[:, :, :3])) > 8 and not np.array_equal(want, plain), "the edge-guided frame shows the plain filter's bytes"

    out = tmp_path / "de"
    r = subprocess.run([str(exe), *args, "--denoise-edges", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    a = np.asarray(Image.open(str(out) + ".png").convert("RGB"))
    assert a.shape == (37, 37, 3) and np.array_equal(a, want[:, :, :3])

    # --denoise alone stays the plain filter
    out0 = tmp_path / "d"
    r = subprocess.run([str(exe), *args, "--denoise", "-o", str(out0)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(str(out0) + ".png").convert("RGB")), plain[:, :, :3])

    # beside --denoise-albedo: both guides, and the knobs reach the filter, --denoise's own among them
    _, want2 = rt.denoise_guided(S, Q, 4, E, 4, albedo_sum=A, albedo_spp=4, rgba8=True, iterations=2, sigma=1.5, sigma_albedo=0.3, sigma_edge=0.2)
    out2 = tmp_path / "de2"
    r = subprocess.run([str(exe), *args, "--denoise-edges", "--denoise-edges-sigma", "0.2", "--denoise-albedo", "--denoise-albedo-sigma", "0.3",
                        "--denoise-iters", "2", "--denoise-sigma", "1.5", "-o", str(out2)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(str(out2) + ".png").convert("RGB")), want2[:, :, :3])
    assert not np.array_equal(want2, want)

    # --adaptive: the adaptive sums, sums of squares and spp map, the ID frame at the maximum spp
    S3, spp, Q3, _ = rt.DeviceScene(hs).render_adaptive(p, min_spp=2, batch_spp=1, rel=0.05)
    _, want3 = rt.denoise_guided(S3, Q3, 0, E, 4, spp_map=spp, rgba8=True)
    out3 = tmp_path / "de3"
    r = subprocess.run([str(exe), *args, "--denoise-edges", "--adaptive", "0.05", "--min-spp", "2", "--batch-spp", "1", "-o", str(out3)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(str(out3) + ".png").convert("RGB")), want3[:, :, :3])


def test_rtrace_refuses_denoise_edges_where_denoise_is_refused_and_a_knob_without_the_flag(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "-o", str(tmp_path / "x")]
    for extra in (["--live"], ["--gpus", "2"], ["--progressive", "2"], ["--orbit", "3"]):
        for flags in (["--denoise-edges"], ["--denoise-edges", "--denoise-albedo"]):
            r = subprocess.run([str(exe), *base, *flags, *extra], capture_output=True, text=True, timeout=60)
            assert r.returncode == 2, (extra, r.returncode, r.stderr)
            assert "--denoise" in r.stderr, (extra, r.stderr)
    for args in ([*base, "--denoise-edges-sigma", "0.3"], [*base, "--denoise", "--denoise-edges-sigma", "0.3"],
                 [*base, "--denoise-albedo", "--denoise-edges-sigma", "0.3"], [*base, "--denoise-edges", "--denoise-edges-sigma", "0"],
                 [*base, "--denoise-edges", "--denoise-edges-sigma"]):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--denoise-edges" in r.stderr, (args, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())
