"""`rtrace --panorama W [--panorama-face F] [--panorama-guard G] [--panorama-at x,y,z]`: the file is, byte for byte, what the Python route
writes — render_panorama, then film or the tone mapper, then the format's writer; and every route the flag cannot go with ends with
status 2 and a message that names both."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGS = ["-s", "6", "--width", "32", "--aspect", "1.0", "--spp", "4", "--depth", "8", "--seed", "5", "--scene-seed", "1"]
AT = (430.0, 450.0, 120.0)


def _rtrace(rt, *args):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    return subprocess.run([str(exe), *ARGS, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def scene(rt):
    hs = rt.HostScene(6, scene_seed=1, width=32, aspect=1.0, spp=4, depth=8)   # cornell_box
    return rt.DeviceScene(hs, device=0)


@pytest.fixture(scope="module")
def pano(scene):
    p = scene.render_panorama(64, center=AT, seed=5)
    assert p.shape == (32, 64, 3) and p.max() > 1.0, "the lamp's radiance is above 1"
    p.setflags(write=False)
    return p


def test_the_hdr_file_is_the_python_routes(rt, gpu, pano, tmp_path):
    r = _rtrace(rt, "--panorama", "64", "--panorama-at", "430,450,120", "--format", "hdr", "-o", str(tmp_path / "cli"))
    assert r.returncode == 0, r.stderr
    rt.write_hdr(tmp_path / "py.hdr", rt.film(pano, 1, "rgbe"))
    assert (tmp_path / "cli.hdr").read_bytes() == (tmp_path / "py.hdr").read_bytes()
    assert (tmp_path / "cli.hdr").read_bytes().startswith(b"#?RADIANCE") and b"-Y 32 +X 64" in (tmp_path / "cli.hdr").read_bytes()[:80]


def test_the_png_behind_the_tone_mapper_is_the_python_routes(rt, gpu, scene, pano, tmp_path):
    from PIL import Image
    r = _rtrace(rt, "--panorama", "64", "--panorama-at", "430,450,120", "--format", "png", "--tonemap", "reinhard", "-o", str(tmp_path / "cli"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "cli.png").convert("RGB")), rt.tonemap(pano, 1, op="reinhard"))
    # the knobs reach the call, and with none of the tone flags the PNG holds the plain output stage's bytes
    other = scene.render_panorama(64, center=AT, face_size=24, guard=2, seed=5)
    assert not np.array_equal(other, pano)
    r = _rtrace(rt, "--panorama", "64", "--panorama-at", "430,450,120", "--panorama-face", "24", "--panorama-guard", "2", "-o", str(tmp_path / "knobs"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "knobs.png").convert("RGB")), rt.tonemap(other, 1))
    # without --panorama-at the point is the scene camera's centre
    r = _rtrace(rt, "--panorama", "16", "--format", "pfm", "-o", str(tmp_path / "own"))
    assert r.returncode == 0, r.stderr
    rt.write_pfm(tmp_path / "py.pfm", rt.film(scene.render_panorama(16, seed=5), 1, "f32"))
    assert (tmp_path / "own.pfm").read_bytes() == (tmp_path / "py.pfm").read_bytes()


def test_what_the_flag_cannot_go_with_ends_with_status_2_and_its_message(rt, gpu, tmp_path):
    out = ["-o", str(tmp_path / "never")]
    for flags, name in ((["--gpus", "2"], "--gpus"), (["--progressive", "2"], "--progressive"), (["--adaptive", "0.05"], "--adaptive"),
                        (["--orbit", "2"], "--orbit"), (["-l"], "--live"), (["--upsample", "2"], "--upsample"), (["--robust", "2"], "--robust"),
                        (["--denoise"], "--denoise"), (["--denoise-albedo"], "--denoise-albedo"), (["--denoise-edges"], "--denoise-edges")):
        r = _rtrace(rt, "--panorama", "64", *flags, *out)
        assert r.returncode == 2, (flags, r.returncode, r.stderr)
        assert "--panorama" in r.stderr and name in r.stderr, (flags, r.stderr)
    for flags in (["--panorama", "63"], ["--panorama", "0"], ["--panorama", "wide"], ["--panorama-face", "18"], ["--panorama", "64", "--panorama-face", "1"],
                  ["--panorama", "64", "--panorama-guard", "-1"], ["--panorama", "64", "--panorama-at", "1,2"], ["--panorama", "64", "--panorama-at", "1,2,x"]):
        r = _rtrace(rt, *flags, *out)
        assert r.returncode == 2 and "--panorama" in r.stderr, (flags, r.returncode, r.stderr)
    r = _rtrace(rt, "--panorama", "64", "--panorama-face", "4", "--panorama-guard", "2", *out)   # the library's own refusal, passed on
    assert r.returncode == 1 and "face_size - 2 * guard" in r.stderr, r.stderr
    assert not any((tmp_path / ("never" + ext)).exists() for ext in (".png", ".hdr", ".pfm"))
