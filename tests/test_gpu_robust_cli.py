"""`rtrace --robust K [--robust-mode M] [--robust-trim T] [--robust-gain X]`: the PNG holds the existing output stage's bytes of the host
mirror's robust means over the K views a Python caller renders; with --denoise, and with --tonemap aces --bloom, the bytes of the Python
composition of the same stages; a K that does not divide spp, and every route the flag cannot go with, ends with an error that says so."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGS = ["-s", "5", "--width", "32", "--aspect", "1.3333333333333333", "--spp", "16", "--depth", "8", "--seed", "5", "--scene-seed", "1"]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(str(path) + ".png").convert("RGB"))


def _rtrace(rt, *args):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    return subprocess.run([str(exe), *ARGS, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def stack(rt):
    """the four sub-frames of `--robust 4 --spp 16 --seed 5`: the camera under seeds 5 .. 8, samples [0, 4)"""
    hs = rt.HostScene(5, scene_seed=1, width=32, aspect=4.0 / 3.0, spp=16, depth=8)   # simple_light
    assert (hs.width, hs.height) == (32, 24)
    s = rt.DeviceScene(hs, device=0).render_views(rt.render_params(sample_end=4), [(hs.camera, 5 + k) for k in range(4)])
    s.setflags(write=False)
    return s


def _display(rt, mean):
    import torch
    d_mean = torch.from_numpy(np.ascontiguousarray(mean)).cuda()
    d_rgba = torch.zeros((24, 32, 4), dtype=torch.uint8, device="cuda")
    rt.resolve_rgba8_device(32, 24, d_mean.data_ptr(), d_rgba.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_rgba.cpu().numpy()[:, :, :3]


def test_the_png_is_the_output_stage_on_the_mirrors_robust_means(rt, gpu, stack, tmp_path):
    want = _display(rt, rt.robust_host(stack, 4))
    plain = _display(rt, np.asarray(stack).sum(axis=0) * (1.0 / 16.0))
    assert len(np.unique(want)) > 8 and not np.array_equal(want, plain), "the estimator must have changed the frame"
    r = _rtrace(rt, "--robust", "4", "-o", str(tmp_path / "gini"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "gini"), want)
    # the knobs reach the call
    for flags, kw in ((["--robust-mode", "median"], dict(mode="median")), (["--robust-mode", "trim", "--robust-trim", "1"], dict(mode="trim", trim=1)),
                      (["--robust-gain", "3.5"], dict(gain=3.5)), (["--robust-mode", "mean"], dict(mode="mean"))):
        r = _rtrace(rt, "--robust", "4", *flags, "-o", str(tmp_path / "knob"))
        assert r.returncode == 0, (flags, r.stderr)
        assert np.array_equal(_png(tmp_path / "knob"), _display(rt, rt.robust_host(stack, 4, **kw))), flags


def test_denoise_and_the_tone_mapping_stages_run_behind_the_combiner(rt, gpu, stack, tmp_path):
    mean, m2 = rt.robust_host(stack, 4, m2=True)
    filtered, rgba = rt.denoise_mean(mean, m2, 4, rgba8=True)
    assert not np.array_equal(rgba[:, :, :3], _display(rt, mean))
    r = _rtrace(rt, "--robust", "4", "--denoise", "-o", str(tmp_path / "dn"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "dn"), rgba[:, :, :3])
    want = rt.tonemap(rt.bloom(mean, 1), 1, op="aces")
    assert not np.array_equal(want, rt.tonemap(mean, 1, op="aces")), "the frame must glow"
    r = _rtrace(rt, "--robust", "4", "--tonemap", "aces", "--bloom", "-o", str(tmp_path / "aces"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "aces"), want)
    r = _rtrace(rt, "--robust", "4", "--denoise", "--tonemap", "aces", "--bloom", "-o", str(tmp_path / "all"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_png(tmp_path / "all"), rt.tonemap(rt.bloom(filtered, 1), 1, op="aces"))


def test_what_the_flag_cannot_go_with_ends_with_an_error_that_names_it(rt, gpu, tmp_path):
    out = ["-o", str(tmp_path / "never")]
    r = _rtrace(rt, "--robust", "3", *out)
    assert r.returncode != 0 and "does not divide" in r.stderr and "16" in r.stderr and "3" in r.stderr, r.stderr
    for flags, name in ((["--orbit", "2"], "--orbit"), (["--adaptive", "0.05"], "--adaptive"), (["-l"], "--live"), (["--upsample", "2"], "--upsample"),
                        (["--denoise-edges"], "--denoise-edges"), (["--denoise-albedo"], "--denoise-albedo"), (["--progressive", "4"], "--progressive"),
                        (["--gpus", "2"], "--gpus")):
        r = _rtrace(rt, "--robust", "4", *flags, *out)
        assert r.returncode == 2, (flags, r.returncode, r.stderr)
        assert "--robust" in r.stderr and name in r.stderr, (flags, r.stderr)
    for flags in (["--robust", "0"], ["--robust", "33"], ["--robust", "four"], ["--robust-mode", "median"], ["--robust", "4", "--robust-mode", "mode"],
                  ["--robust", "4", "--robust-gain", "0"], ["--robust", "4", "--robust-gain", "nan"], ["--robust", "4", "--robust-trim", "-1"]):
        r = _rtrace(rt, *flags, *out)
        assert r.returncode == 2, (flags, r.returncode, r.stderr)
    assert not (tmp_path / "never.png").exists()
