"""The denoiser's C ABI without a GPU: the five symbols and their Rust declarations, the layout and the sized initialiser of
rt_denoise_params, the workspace size, and every invalid argument of rt_denoise_device and rt_render_moments[_device] (checked before
the scene handle and the device, the field named).  The numpy restatement that tests/test_gpu_denoise.py holds the device to is
checked here against exact rational arithmetic on one pixel."""
import ctypes as C
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import denoise_helpers

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_render_moments_device", "rt_render_moments", "rt_denoise_params_init_sized", "rt_denoise_workspace_bytes", "rt_denoise_device")


def test_the_symbols_are_exported_declared_and_bound(rt):
    lib = rt.amd_lib()
    header = (ROOT / "include" / "rt_amd.h").read_text()
    text = (ROOT / "INTEGRATION.md").read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_amd.so")], check=True, capture_output=True, text=True).stdout
    for fn in SYMBOLS:
        assert getattr(lib, fn) is not None
        assert fn in rt.RT_AMD_SYMBOLS, fn
        assert re.search(r"\b(int|int64_t) " + fn + r"\(", header), fn
        assert f"pub fn {fn}(" in text, fn
        assert re.search(r" T " + fn + r"$", exported, flags=re.M), fn
    assert "pub struct rt_denoise_params" in text
    for name in ("render_moments", "render_moments_device"):
        assert callable(getattr(rt.DeviceScene, name))
    assert callable(rt.denoise_device) and callable(rt.denoise) and callable(rt.denoise_params)


def test_rt_denoise_params_has_gccs_layout_and_its_rust_fields(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(rt_denoise_params));']
    for fname, _ in rt.DenoiseParams._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rt_denoise_params, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(rt.DenoiseParams) == 24
    for fname, _ in rt.DenoiseParams._fields_:
        assert int(got[fname]) == getattr(rt.DenoiseParams, fname).offset, fname
    text = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"pub struct rt_denoise_params\s*\{(.*?)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in rt.DenoiseParams._fields_]


def test_init_sized_writes_the_defaults_into_struct_size_bytes_only(rt):
    lib = rt.amd_lib()
    d = rt.denoise_params()
    assert (d.struct_size, d.iterations, d.sigma, d.eps) == (24, 4, 4.0, 1e-6)
    assert denoise_helpers.DEFAULTS == dict(iterations=d.iterations, sigma=d.sigma, eps=d.eps)
    for size in (8, 16, 24):
        buf = (C.c_uint8 * 40)(*([0xA5] * 40))
        assert lib.rt_denoise_params_init_sized(buf, size) == 0
        raw = bytes(buf)
        assert raw[size:] == b"\xa5" * (40 - size), size
        assert raw[:size] == bytes(rt.DenoiseParams(struct_size=size, iterations=4, sigma=4.0, eps=1e-6))[:size], size
    for size in (0, 4, 12, 20, 25, 32):
        buf = (C.c_uint8 * 40)(*([0xA5] * 40))
        assert lib.rt_denoise_params_init_sized(buf, size) == -1, size
        assert "struct_size" in lib.rt_last_error().decode()
        assert bytes(buf) == b"\xa5" * 40
    assert lib.rt_denoise_params_init_sized(None, 24) == -1
    with pytest.raises(TypeError):
        rt.denoise_params(radius=3)


def test_the_workspace_is_positive_and_grows_with_the_frame(rt):
    lib = rt.amd_lib()
    sizes = [(1, 1), (5, 3), (17, 9), (70, 37), (130, 66), (256, 256), (1200, 800)]
    got = [lib.rt_denoise_workspace_bytes(w, h) for w, h in sizes]
    assert all(b > 0 for b in got)
    assert got == sorted(got) and len(set(got)) == len(got)
    for (w, h), b in zip(sizes, got):
        assert b >= 2 * 4 * 8 * w * h, "two halves of four doubles per pixel"
        assert lib.rt_denoise_workspace_bytes(h, w) == b, "a function of w * h"
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 14, 1 << 13)):
        assert lib.rt_denoise_workspace_bytes(w, h) < 0
        with pytest.raises(rt.RtError):
            rt.denoise_workspace_bytes(w, h)


def _denoise(rt, *, w=6, h=4, s=True, q=True, spp=8, spp_map=False, params=None, out=True, rgba=True, ws=True, alias=None, misalign=False,
             ws_misalign=False):
    """One call of rt_denoise_device on HOST buffers: only argument checks can answer (the first thing past them asks the HIP runtime
    which device owns d_mean_out, and host memory has none)."""
    lib = rt.amd_lib()
    n = w * h if w > 0 and h > 0 else 1
    S, Q, M = (C.c_double * (3 * n))(), (C.c_double * (3 * n))(), (C.c_double * (3 * n))()
    N = (C.c_int32 * n)()
    B = (C.c_uint8 * (4 * n + 4))()
    W = (C.c_uint8 * (64 * n + 32))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    out_ptr = C.addressof(M)
    if alias == "sum":
        out_ptr = C.addressof(S) + 8 * (3 * n - 1)   # the last double of S
    elif alias == "sum_sq":
        out_ptr = C.addressof(Q)
    rc = lib.rt_denoise_device(w, h, C.addressof(S) if s else None, C.addressof(Q) if q else None, spp, C.addressof(N) if spp_map else None,
                               C.byref(params) if params is not None else None, out_ptr if out else None,
                               (C.addressof(B) + (1 if misalign else 0)) if rgba else None, ws_ptr if ws else None, None)
    return rc, lib.rt_last_error().decode()


def test_every_invalid_denoise_argument_is_named_without_a_device(rt):
    P = rt.DenoiseParams
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(s=False), "d_sum is null"),
        (dict(q=False), "d_sum_sq is null"),
        (dict(out=False), "d_mean_out is null"),
        (dict(ws=False), "d_workspace is null"),
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(spp=1), "spp"), (dict(spp=0), "spp"), (dict(spp=-4), "spp"),
        (dict(params=P(struct_size=12, iterations=4, sigma=4.0, eps=1e-6)), "struct_size"),
        (dict(params=P(struct_size=32, iterations=4, sigma=4.0, eps=1e-6)), "struct_size"),
        (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=rt.denoise_params(iterations=0)), "iterations"),
        (dict(params=rt.denoise_params(iterations=7)), "iterations"),
        (dict(params=rt.denoise_params(iterations=-1)), "iterations"),
        (dict(params=rt.denoise_params(sigma=0.0)), "sigma"), (dict(params=rt.denoise_params(sigma=-1.0)), "sigma"),
        (dict(params=rt.denoise_params(sigma=nan)), "sigma"), (dict(params=rt.denoise_params(sigma=inf)), "sigma"),
        (dict(params=rt.denoise_params(eps=0.0)), "eps"), (dict(params=rt.denoise_params(eps=-1e-6)), "eps"),
        (dict(params=rt.denoise_params(eps=nan)), "eps"),
        (dict(alias="sum"), "d_mean_out"), (dict(alias="sum_sq"), "d_mean_out"),
        (dict(misalign=True), "d_rgba8"),
        (dict(ws_misalign=True), "d_workspace"),
    ]
    for kw, field in cases:
        rc, msg = _denoise(rt, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith("rt_denoise_device: "), (kw, msg)
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(rgba=False), dict(spp=1, spp_map=True), dict(spp=2), dict(params=rt.denoise_params(iterations=6)),
               dict(params=rt.denoise_params(iterations=1, sigma=0.5, eps=1e-12)),
               dict(params=P(struct_size=8, iterations=2)), dict(params=P(struct_size=16, iterations=2, sigma=1.0))):
        rc, msg = _denoise(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)
    # a shorter struct's missing fields are the defaults, not the bytes behind it: eps = 0 beyond struct_size 16 is not looked at
    rc, msg = _denoise(rt, params=P(struct_size=16, iterations=2, sigma=1.0, eps=0.0))
    assert "not a device pointer" in msg, msg


@pytest.mark.parametrize("device", [False, True])
def test_every_invalid_moments_argument_is_named_before_the_scene_is_looked_at(rt, device):
    lib = rt.amd_lib()
    hs = rt.HostScene(6, width=16, spp=8, depth=4)
    n = hs.width * hs.height
    S, Q = (C.c_double * (3 * n))(), (C.c_double * (3 * n))()
    big = rt.Camera.from_buffer_copy(hs.camera)
    big.image_width, big.image_height = 1 << 14, 1 << 13

    def call(*, params=None, camera=hs.camera, s=True, q=True):
        p = params if params is not None else rt.render_params(seed=1)
        args = [None, C.byref(camera) if camera is not None else None, C.byref(p) if p is not False else None,
                C.addressof(S) if s else None, C.addressof(Q) if q else None]
        rc = lib.rt_render_moments_device(*args, None) if device else lib.rt_render_moments(*args)
        return rc, lib.rt_last_error().decode()

    cases = [
        (dict(camera=None), "camera"),
        (dict(params=False), "params"),
        (dict(s=False), "d_sum is null" if device else "sum is null"),
        (dict(q=False), "d_sum_sq is null" if device else "sum_sq is null"),
        (dict(params=rt.render_params(shard_count=2)), "shard_count"),
        (dict(params=rt.render_params(shard_count=2, shard_index=1)), "shard_count"),
        (dict(params=rt.render_params(out_layout=rt.RT_OUT_TILES)), "out_layout"),
        (dict(camera=big), "image_width"),
        (dict(), "scene"),
        (dict(params=rt.render_params(accumulate=True, sample_begin=2, sample_end=5)), "scene"),
    ]
    for kw, field in cases:
        rc, msg = call(**kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg, (kw, msg)
    for kw, _ in cases[:7] + cases[8:]:
        assert call(**kw)[1].startswith("rt_render_moments_device: " if device else "rt_render_moments: "), kw


def _r(x):
    return float(x)  # Fraction -> the nearest double, ties to even: one correctly rounded operation


def test_the_numpy_statement_is_the_definition_rounded_once_per_operation():
    """A 1 x 1 frame: one tap, the centre.  Exact rational arithmetic rounded after every operation gives the prepared mean and
    variance, and one iteration gives C = (w * m) / w and V = ((w * w) * V0) / (w * w) with w = 9/64 — which need not be m and V0."""
    S, Q, n = [0.7, 2.3, 1.1], [0.41, 1.9, 0.52], 3
    m = [_r(Fraction(s) / n) for s in S]
    v = [_r(Fraction(_r(Fraction(q) - Fraction(_r(Fraction(s) * Fraction(mc))))) / (n - 1)) for s, q, mc in zip(S, Q, m)]
    V0 = _r(Fraction(max(max(v), 0.0)) / n)
    C0, Vp, valid = denoise_helpers.prepare(np.array([[S]]), np.array([[Q]]), n)
    assert valid.all() and [float(x).hex() for x in C0[0, 0]] == [x.hex() for x in m] and float(Vp[0, 0]).hex() == V0.hex()
    w = 9.0 / 64.0
    want_c = [_r(Fraction(_r(Fraction(w) * Fraction(mc))) / Fraction(w)) for mc in m]
    want_v = _r(Fraction(_r(Fraction(_r(Fraction(w) * Fraction(w))) * Fraction(V0))) / Fraction(_r(Fraction(w) * Fraction(w))))
    C1, V1 = denoise_helpers.iterate(C0, Vp, valid, 1, 4.0, 1e-6)
    assert [float(x).hex() for x in C1[0, 0]] == [x.hex() for x in want_c] and float(V1[0, 0]).hex() == want_v.hex()
    # a pixel that is not valid keeps its mean and is no tap: the neighbour filters alone
    S2, Q2 = np.array([[S, [np.nan, 1.0, 1.0]]]), np.array([[Q, [1.0, 1.0, 1.0]]])
    out = denoise_helpers.denoise(S2, Q2, n, iterations=3)
    assert [float(x).hex() for x in out[0, 0]] == [float(x).hex() for x in denoise_helpers.denoise(np.array([[S]]), np.array([[Q]]), n, iterations=3)[0, 0]]
    assert np.isnan(out[0, 1, 0]) and out[0, 1, 1] == 1.0 / 3.0
    # n < 2 is not valid either, whatever the moments say
    assert not denoise_helpers.prepare(np.array([[S]]), np.array([[Q]]), np.array([[1]]))[2].any()
