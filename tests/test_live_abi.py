"""Live refinement's C ABI without a GPU: the three symbols and their Rust declarations, every invalid argument (checked before the
scene handle and the device, the field named), the command line's refusals, and the rounding order of the running-mean recurrence
that tests/test_gpu_live.py holds the device to."""
import ctypes as C
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import live_helpers

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_render_mean_device", "rt_render_mean", "rt_resolve_rgba8_device")


def test_the_three_symbols_are_exported_declared_and_bound(rt):
    lib = rt.amd_lib()
    header = (ROOT / "include" / "rt_amd.h").read_text()
    text = (ROOT / "INTEGRATION.md").read_text()
    for fn in SYMBOLS:
        assert getattr(lib, fn) is not None
        assert fn in rt.RT_AMD_SYMBOLS, fn
        assert f"int {fn}(" in header, fn
        assert f"pub fn {fn}(" in text, fn
    assert callable(rt.DeviceScene.render_mean) and callable(rt.DeviceScene.render_mean_device) and callable(rt.resolve_rgba8_device)


def _call(rt, *, params=None, camera=True, mean=True, rgba8=True, device=False, misalign=False):
    """One call of rt_render_mean (or its device form) with a NULL scene: only argument checks can answer."""
    lib = rt.amd_lib()
    hs = rt.HostScene(6, width=16, spp=8, depth=4)
    cam = hs.camera
    p = params if params is not None else rt.render_params(seed=1)
    n = cam.image_width * cam.image_height
    out_mean = (C.c_double * (3 * n))()
    out_rgba = (C.c_uint8 * (4 * n + 4))()
    args = [None, C.byref(cam) if camera else None, C.byref(p) if p is not False else None,
            C.addressof(out_mean) if mean else None, (C.addressof(out_rgba) + (1 if misalign else 0)) if rgba8 else None]
    rc = lib.rt_render_mean_device(*args, None) if device else lib.rt_render_mean(*args)
    return rc, lib.rt_last_error().decode()


@pytest.mark.parametrize("device", [False, True])
def test_every_invalid_live_argument_is_named_before_the_scene_is_looked_at(rt, device):
    cases = [
        (dict(camera=False), "camera"),
        (dict(params=False), "params"),
        (dict(mean=False), "d_mean" if device else "mean"),
        (dict(params=rt.render_params(accumulate=True)), "accumulate"),
        (dict(params=rt.render_params(shard_count=2)), "shard_count"),
        (dict(params=rt.render_params(shard_count=2, shard_index=1)), "shard_count"),
        (dict(params=rt.render_params(out_layout=rt.RT_OUT_TILES)), "out_layout"),
        (dict(params=rt.render_params(sample_begin=-1)), "sample_begin"),
        (dict(params=rt.render_params(sample_begin=3, sample_end=3)), "sample_begin, sample_end"),
        (dict(params=rt.render_params(sample_begin=5, sample_end=2)), "sample_begin, sample_end"),
        (dict(params=rt.render_params(sample_begin=8)), "sample_begin, sample_end"),  # sample_end 0: the camera's 8 spp, so [8, 8)
        (dict(), "scene"),             # every other argument is fine: the null scene is what is left
        (dict(rgba8=False), "scene"),  # the display frame is optional
        (dict(params=rt.render_params(sample_begin=7)), "scene"),  # [7, 8) of the camera's 8 spp is a range
    ]
    if device:
        cases.append((dict(misalign=True), "d_rgba8"))  # the device form stores one 4-byte word per pixel
    for kw, field in cases:
        rc, msg = _call(rt, device=device, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg, (kw, msg)
        assert msg.startswith("rt_render_mean_device: " if device else "rt_render_mean: "), (kw, msg)


def test_resolve_rgba8_device_rejects_bad_arguments_without_a_gpu(rt):
    lib = rt.amd_lib()
    buf = (C.c_double * 12)()
    out = (C.c_uint8 * 20)()
    for args in ((2, 2, None, C.addressof(out)), (2, 2, C.addressof(buf), None), (0, 2, C.addressof(buf), C.addressof(out)),
                 (2, -1, C.addressof(buf), C.addressof(out)), (2, 2, C.addressof(buf), C.addressof(out) + 2)):
        assert lib.rt_resolve_rgba8_device(*args, None) == -1, args
        assert b"rt_resolve_rgba8_device" in lib.rt_last_error()


def test_rtrace_refuses_live_with_what_it_cannot_be_combined_with(rt, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "-o", str(tmp_path / "x")]
    for live in ("-l", "--live"):
        for extra in (["--gpus", "2"], ["--progressive", "2"], ["--adaptive", "0.05"], ["--orbit", "3"]):
            r = subprocess.run([str(exe), *base, live, *extra], capture_output=True, text=True, timeout=60)
            assert r.returncode == 2, (extra, r.returncode, r.stderr)
            assert "--live" in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    for args in ([*base, "--live", "--live-spp", "0"], [*base, "--live-spp", "2"], ["-s", "6", "--live"]):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "live" in r.stderr, (args, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def _round(x):
    return float(x)  # Fraction -> the nearest double, ties to even: one correctly rounded operation


def test_the_recurrence_is_three_separately_rounded_operations_with_a_true_division():
    """Samples 0.408, 0.045, 0.049 of one value: at the third, (c - m) / 3 and (c - m) * (1.0 / 3) differ in the last bit, and so do the
    means.  The numpy statement the GPU tests use must give what exact rational arithmetic, rounded once per operation, gives."""
    c = [0.408, 0.045, 0.049]
    m = 0.0
    for s, x in enumerate(c):
        d = _round(Fraction(x) - Fraction(m))
        q = _round(Fraction(d) / (s + 1))
        m = _round(Fraction(m) + Fraction(q))
    assert m.hex() == "0x1.56b2dbd194237p-3"
    got = live_helpers.fold([np.array([x]) for x in c])
    assert float(got[0]).hex() == m.hex()
    m2 = float(live_helpers.fold([np.array([x]) for x in c[:2]])[0])
    d = c[2] - m2
    assert abs(np.float64(d / 3.0).view(np.int64) - np.float64(d * (1.0 / 3.0)).view(np.int64)) == 1
    assert float(live_helpers.fold_by_reciprocal([np.array([x]) for x in c])[0]).hex() == "0x1.56b2dbd194238p-3"
    # continuing after two samples is the same as folding all three; and neither is sum / n
    assert float(live_helpers.fold([np.array([c[2]])], mean=np.array([m2]), first=2)[0]).hex() == m.hex()
    assert ((c[0] + c[1]) + c[2]) / 3.0 != m
