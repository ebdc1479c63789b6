"""`rtrace --compare REF.pfm` and `rtrace -l --live-stop X`: the frame metrics of include/rt_amd.h behind the command line.  The printed
doubles (%.17g) are compared bit for bit with the host mirror on the frames the Python routes give, and the live loop's stop with
DeviceScene.render_until's."""
import re
import subprocess

import numpy as np
import pytest

import metrics_helpers as mh

pytestmark = pytest.mark.gpu

SCENE = ["-s", "5", "--width", "24", "--aspect", "1.5", "--depth", "8", "--scene-seed", "1"]
W, H = 24, 16


def _run(rt, *args):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    return subprocess.run([str(exe), *SCENE, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


def _metrics(stdout):
    lines = [line for line in stdout.splitlines() if line.startswith("metrics: ")]
    assert len(lines) == 1, stdout
    got = dict(kv.split("=") for kv in lines[0].split()[1:])
    assert list(got) == ["count", "mse", "rmse", "relmse", "mae", "bias", "max", "psnr"], lines[0]
    names = dict(relmse="rel_mse", max="max_abs")
    return {names.get(k, k): float(v) for k, v in got.items()}


@pytest.fixture(scope="module")
def scene(rt):
    hs = rt.HostScene(5, scene_seed=1, width=W, aspect=1.5, spp=12, depth=8)
    assert (hs.width, hs.height) == (W, H)
    return hs, rt.DeviceScene(hs, device=0)


def test_compare_prints_the_mirrors_doubles(rt, gpu, scene, tmp_path):
    hs, ds = scene
    ref_name = tmp_path / "ref"
    r = _run(rt, "--spp", 48, "--seed", 4, "--format", "pfm", "-o", ref_name)
    assert r.returncode == 0, r.stderr
    ref = rt.read_pfm(str(ref_name) + ".pfm")
    assert ref.shape == (H, W, 3)
    # the file holds the 48-spp means as f32
    sums48 = ds.render(rt.render_params(seed=4, sample_end=48)).reshape(H, W, 3)
    assert np.array_equal(mh.bits(ref), mh.bits((sums48 * (1.0 / 48.0)).astype(np.float32).astype(np.float64)))

    # a plain render: its sums with the count
    sums = ds.render(rt.render_params(seed=3)).reshape(H, W, 3)
    r = _run(rt, "--spp", 12, "--seed", 3, "--compare", str(ref_name) + ".pfm", "-o", tmp_path / "plain")
    assert r.returncode == 0, r.stderr
    want = rt.frame_error_host(sums, 12, ref, 1)
    assert want["count"] == W * H and want["mse"] > 0.0
    assert mh.same_bits(_metrics(r.stdout), want, mh.ERROR_FIELDS), (r.stdout, want)
    # ... with another eps, and with the tone mapping on, which runs behind the measurement
    r = _run(rt, "--spp", 12, "--seed", 3, "--compare", str(ref_name) + ".pfm", "--compare-eps", "1e-4", "--tonemap", "aces", "-o", tmp_path / "toned")
    assert r.returncode == 0, r.stderr
    assert mh.same_bits(_metrics(r.stdout), rt.frame_error_host(sums, 12, ref, 1, eps=1e-4), mh.ERROR_FIELDS)
    # the denoised route: the filtered means, on the device
    S, Q = ds.render_moments(rt.render_params(seed=3))
    filtered = rt.denoise(S, Q, 12)
    r = _run(rt, "--spp", 12, "--seed", 3, "--denoise", "--compare", str(ref_name) + ".pfm", "-o", tmp_path / "filtered")
    assert r.returncode == 0, r.stderr
    want = rt.frame_error_host(filtered, 1, ref, 1)
    assert mh.same_bits(_metrics(r.stdout), want, mh.ERROR_FIELDS), (r.stdout, want)
    # the frame against its own file: only the rounding to f32 is left
    r = _run(rt, "--spp", 48, "--seed", 4, "--compare", str(ref_name) + ".pfm", "-o", tmp_path / "same")
    assert r.returncode == 0, r.stderr
    assert mh.same_bits(_metrics(r.stdout), rt.frame_error_host(sums48, 48, ref, 1), mh.ERROR_FIELDS)
    assert _metrics(r.stdout)["max_abs"] < 1e-5


def test_compare_refuses_what_it_cannot_measure(rt, gpu, tmp_path):
    ref_name = tmp_path / "ref"
    assert _run(rt, "--spp", 2, "--format", "pfm", "-o", ref_name).returncode == 0
    ref = str(ref_name) + ".pfm"
    out = tmp_path / "out"
    for flags in (["-l"], ["--orbit", 2], ["--progressive", 1], ["--gpus", 2]):
        r = _run(rt, "--spp", 2, "--compare", ref, "-o", out, *flags)
        assert r.returncode != 0 and "--compare" in r.stderr and "cannot be combined" in r.stderr, (flags, r.stderr)
        assert "metrics:" not in r.stdout
    r = _run(rt, "--spp", 2, "--compare-eps", "0.1", "-o", out)
    assert r.returncode != 0 and "--compare" in r.stderr
    r = _run(rt, "--spp", 2, "--compare", ref, "--compare-eps", "0", "-o", out)
    assert r.returncode != 0 and "--compare-eps" in r.stderr
    # a reference of another size, a file that is no PFM, no file at all: an error, not a frame
    exe = rt.LIB_DIR / "rtrace"
    r = subprocess.run([str(exe), "-s", "5", "--width", "30", "--aspect", "1.5", "--depth", "8", "--spp", "2", "--compare", ref, "-o", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "24 x 16" in r.stderr and "30 x 20" in r.stderr, r.stderr
    bad = tmp_path / "bad.pfm"
    bad.write_bytes(b"PF\n24 16\n0.0\n" + bytes(24 * 16 * 12))
    r = _run(rt, "--spp", 2, "--compare", bad, "-o", out)
    assert r.returncode != 0 and "scale" in r.stderr, r.stderr
    r = _run(rt, "--spp", 2, "--compare", tmp_path / "none.pfm", "-o", out)
    assert r.returncode != 0 and "cannot open" in r.stderr, r.stderr
    r = _run(rt, "--spp", 2, "--live-stop", "0.1", "-o", out)
    assert r.returncode != 0 and "--live-stop" in r.stderr
    r = _run(rt, "--spp", 2, "-l", "--live-stop-min", 4, "-o", out)
    assert r.returncode != 0 and "--live-stop-min" in r.stderr


def test_live_stop_ends_where_render_until_does(rt, gpu, scene, tmp_path):
    hs, ds = scene
    seed, floor, spp = 3, 5, 13     # the live loop settles on spp - 1 = 12 samples (the reference loop's convention)
    noises = []
    mean = m2 = None
    for s in range(spp - 1):
        mean, m2 = ds.render_mean_moments(rt.render_params(seed=seed, sample_begin=s, sample_end=s + 1), mean=mean, m2=m2)
        noises.append(rt.frame_noise_host(mean, m2, s + 1, form="means")["noise"])
    # a condition of the test: a pass strictly between the floor and the end whose noise is below every earlier pass's from the floor on
    stop = next((n for n in range(floor + 1, spp - 1) if noises[n - 1] < min(noises[floor - 1:n - 1])), None)
    assert stop is not None, noises
    threshold = noises[stop - 1]
    _, _, samples, noise = ds.render_until(threshold, max_spp=spp - 1, min_samples=floor, seed=seed)
    assert samples == stop

    r = _run(rt, "--spp", spp, "--seed", seed, "-l", "--live-stop", repr(threshold), "--live-stop-min", floor, "-o", tmp_path / "stopped")
    assert r.returncode == 0, r.stderr
    assert f"Live: {stop} frames, {stop} samples per pixel in the last" in r.stdout, r.stdout
    passes = re.findall(r"^live-stop-pass: samples=(\d+) noise=(\S+)$", r.stdout, flags=re.M)
    assert [int(n) for n, _ in passes] == list(range(1, stop + 1))
    assert np.array_equal(mh.bits([float(x) for _, x in passes]), mh.bits(noises[:stop])), "every pass's noise is the mirror's"
    final = re.findall(r"^live-stop: samples=(\d+) noise=(\S+)$", r.stdout, flags=re.M)
    assert len(final) == 1 and int(final[0][0]) == stop and mh.bits(float(final[0][1])) == mh.bits(noise)
    # the frame written is the plain live route's at that many samples
    r = _run(rt, "--spp", stop + 1, "--seed", seed, "-l", "-o", tmp_path / "plain")
    assert r.returncode == 0, r.stderr
    assert "live-stop" not in r.stdout
    assert (tmp_path / "stopped.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    # a threshold nothing reaches: the loop runs to spp - 1 as without the flag, with the same frame
    r = _run(rt, "--spp", stop + 1, "--seed", seed, "-l", "--live-stop", 0, "-o", tmp_path / "full")
    assert r.returncode == 0, r.stderr
    assert f"live-stop: samples={stop} " in r.stdout
    assert (tmp_path / "full.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    # ... and in a film format the stopped frame is the means of that pass
    r = _run(rt, "--spp", spp, "--seed", seed, "-l", "--live-stop", repr(threshold), "--live-stop-min", floor, "--format", "pfm", "-o", tmp_path / "film")
    assert r.returncode == 0, r.stderr
    want, _ = ds.render_mean_moments(rt.render_params(seed=seed, sample_end=stop))
    assert np.array_equal(mh.bits(rt.read_pfm(tmp_path / "film.pfm")), mh.bits(want.astype(np.float32).astype(np.float64)))
