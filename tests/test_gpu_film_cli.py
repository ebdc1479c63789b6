"""`rtrace --format png|png16|hdr|pfm`: the file, read back by the readers in tests/film_helpers.py, holds the film stage's host mirror
of the route's own sums or means — plain, behind --tonemap / --exposure / --bloom, on a device route, per --orbit view and for the last
frame of -l; the default format still writes the 8-bit PNG it wrote; and what the flag cannot go with ends with status 2, both flags named."""
import subprocess

import numpy as np
import pytest

import film_helpers as fh

pytestmark = pytest.mark.gpu

ARGS = ["-s", "5", "--width", "24", "--aspect", "1.5", "--spp", "6", "--depth", "8", "--seed", "5", "--scene-seed", "1"]
W, H, SPP = 24, 16, 6


def _rtrace(rt, *args):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    return subprocess.run([str(exe), *ARGS, *args], capture_output=True, text=True, timeout=300)


def _read(path, fmt):
    """the file rtrace wrote for `fmt`, as film_helpers' bits"""
    if fmt == "hdr":
        return fh.read_hdr(str(path) + ".hdr")[0]
    if fmt == "pfm":
        return fh.read_pfm(str(path) + ".pfm")
    return fh.read_png16(str(path) + ".png")[0]


FILM = {"hdr": fh.RGBE, "pfm": fh.F32, "png16": fh.RGB16}


def _want(rt, values, spp, fmt, **kw):
    return fh.as_bits(FILM[fmt], rt.film_host(values, spp, FILM[fmt], **kw))


@pytest.fixture(scope="module")
def scene(rt):
    hs = rt.HostScene(5, scene_seed=1, width=W, aspect=1.5, spp=SPP, depth=8)   # simple_light: an emitter of radiance 4
    assert (hs.width, hs.height) == (W, H)
    return hs, rt.DeviceScene(hs, device=0)


@pytest.fixture(scope="module")
def sums(rt, scene):
    s = scene[1].render(rt.render_params(seed=5)).reshape(H, W, 3)
    assert s.max() / SPP > 1.0, "the frame must hold radiance above 1"
    s.setflags(write=False)
    return s


@pytest.mark.parametrize("fmt", ["hdr", "pfm", "png16"])
def test_a_plain_render_in_every_format(rt, gpu, sums, tmp_path, fmt):
    r = _rtrace(rt, "--format", fmt, "-o", str(tmp_path / "plain"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_read(tmp_path / "plain", fmt), _want(rt, sums, SPP, fmt))
    if fmt == "pfm":   # with no tone flag the linear formats hold the means, unclipped
        assert np.array_equal(_read(tmp_path / "plain", fmt), (sums * (1.0 / SPP)).astype(np.float32).view(np.uint32))
        assert _read(tmp_path / "plain", fmt).view(np.float32).max() > 1.0
    # the tone flags and bloom apply in front of the format: --exposure is in stops
    r = _rtrace(rt, "--format", fmt, "--tonemap", "reinhard", "--exposure", "1", "--bloom", "-o", str(tmp_path / "toned"))
    assert r.returncode == 0, r.stderr
    bloomed = rt.bloom_host(sums, SPP, strength=0.25)
    want = _want(rt, bloomed, 1, fmt, op="reinhard", exposure=2.0)
    assert not np.array_equal(want, _want(rt, sums, SPP, fmt, op="reinhard", exposure=2.0)), "the frame must glow"
    assert np.array_equal(_read(tmp_path / "toned", fmt), want)


def test_the_default_format_writes_the_png_it_wrote(rt, gpu, sums, tmp_path):
    from PIL import Image
    a = _rtrace(rt, "-o", str(tmp_path / "none"))
    b = _rtrace(rt, "--format", "png", "-o", str(tmp_path / "png"))
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert (tmp_path / "none.png").read_bytes() == (tmp_path / "png.png").read_bytes()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "none.png").convert("RGB")), rt.resolve_rgb8_host(W, H, SPP, sums))
    c = _rtrace(rt, "--format", "png16", "-o", str(tmp_path / "deep"))      # and the 16-bit file's high bytes are that PNG's
    assert c.returncode == 0, c.stderr
    assert np.array_equal(fh.read_png16(tmp_path / "deep.png")[0] >> 8, rt.resolve_rgb8_host(W, H, SPP, sums))


def test_the_device_routes_write_the_format_too(rt, gpu, scene, tmp_path):
    hs, ds = scene
    S, Q = ds.render_moments(rt.render_params(seed=5, sample_end=SPP))
    mean, _ = rt.denoise(S, Q, SPP, rgba8=True)
    r = _rtrace(rt, "--denoise", "--format", "pfm", "-o", str(tmp_path / "dn"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_read(tmp_path / "dn", "pfm"), _want(rt, mean, 1, "pfm"))
    r = _rtrace(rt, "--denoise", "--format", "hdr", "--tonemap", "aces", "--auto-exposure", "-o", str(tmp_path / "dn"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_read(tmp_path / "dn", "hdr"), _want(rt, mean, 1, "hdr", op="aces", auto_key=0.18))
    # every view of an orbit is a file of its own
    views = rt.orbit_views(hs, 2, seed=5)
    frames = ds.render_views(rt.render_params(seed=5), views).reshape(2, H, W, 3)
    r = _rtrace(rt, "--orbit", "2", "--format", "hdr", "-o", str(tmp_path / "orbit"))
    assert r.returncode == 0, r.stderr
    for k in range(2):
        assert np.array_equal(_read(tmp_path / f"orbit_{k:03d}", "hdr"), _want(rt, frames[k], SPP, "hdr")), k
    # the last frame of -l: the running mean of spp - 1 samples
    live = ds.render_mean(rt.render_params(seed=5, sample_end=SPP - 1))
    r = _rtrace(rt, "-l", "--format", "png16", "--exposure", "-1", "-o", str(tmp_path / "live"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_read(tmp_path / "live", "png16"), _want(rt, live, 1, "png16", exposure=0.5))


def test_what_the_flag_cannot_go_with_ends_with_status_2_and_names_both_flags(rt, gpu, tmp_path):
    out = ["-o", str(tmp_path / "never")]
    for flags, other in ((["--format", "hdr", "--gpus", "2"], "--gpus"), (["--format", "pfm", "--progressive", "2"], "--progressive"),
                         (["--format", "png16", "--gpus", "2"], "--gpus")):
        r = _rtrace(rt, *flags, *out)
        assert r.returncode == 2, (flags, r.returncode, r.stderr)
        assert "--format" in r.stderr and other in r.stderr, (flags, r.stderr)
        assert not any((tmp_path / ("never" + ext)).exists() for ext in (".png", ".hdr", ".pfm")), flags
    r = _rtrace(rt, "--format", "exr", *out)
    assert r.returncode == 2 and "--format" in r.stderr
