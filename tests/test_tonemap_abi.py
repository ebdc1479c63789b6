"""The tone-mapping stage's C ABI without a GPU: the symbols and their Rust declarations, the layout and the sized initialiser of
rt_tonemap_params, the workspace size, and every invalid argument of rt_tonemap_device and rt_log_average_luminance_device (checked
before any device work, the field named)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

import tonemap_helpers as th

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_tonemap_params_init_sized", "rt_tonemap_workspace_bytes", "rt_tonemap_device", "rt_log_average_luminance_device")
HOST_SYMBOLS = ("rth_tonemap", "rth_log_average_luminance")


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
    assert "pub struct rt_tonemap_params" in text
    assert "tone mapping (opt-in; nothing above changes)" in header
    assert re.search(r"#define RT_ABI_VERSION 2\b", header)
    host_header = (ROOT / "include" / "rt_host.h").read_text()
    for fn in HOST_SYMBOLS:
        assert fn in rt.RT_HOST_SYMBOLS and re.search(r"\bint " + fn + r"\(", host_header), fn
    for name in ("tonemap_params", "tonemap_workspace_bytes", "tonemap_device", "log_average_luminance_device", "tonemap", "log_average_luminance",
                 "tonemap_host", "log_average_luminance_host"):
        assert callable(getattr(rt, name)), name
    assert (rt.RT_TONEMAP_CLAMP, rt.RT_TONEMAP_REINHARD, rt.RT_TONEMAP_ACES) == (0, 1, 2) == th.OPS
    for name, value in (("CLAMP", 0), ("REINHARD", 1), ("ACES", 2)):
        assert re.search(rf"#define RT_TONEMAP_{name} {value}\b", header)


def test_rt_tonemap_params_has_gccs_layout_and_its_rust_fields(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(rt_tonemap_params));']
    for fname, _ in rt.TonemapParams._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rt_tonemap_params, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(rt.TonemapParams) == 40
    for fname, _ in rt.TonemapParams._fields_:
        assert int(got[fname]) == getattr(rt.TonemapParams, fname).offset, fname
    text = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"pub struct rt_tonemap_params\s*\{(.*?)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in rt.TonemapParams._fields_]


def test_init_sized_writes_the_defaults_into_struct_size_bytes_only(rt):
    lib = rt.amd_lib()
    t = rt.tonemap_params()
    assert (t.struct_size, t.op, t.exposure, t.auto_key, t.delta, t.white) == (40, 0, 1.0, 0.0, 1e-4, th.INF)
    assert th.DEFAULTS == dict(op=t.op, exposure=t.exposure, auto_key=t.auto_key, delta=t.delta, white=t.white)
    for size in (8, 16, 24, 32, 40):
        buf = (C.c_uint8 * 56)(*([0xA5] * 56))
        assert lib.rt_tonemap_params_init_sized(buf, size) == 0
        raw = bytes(buf)
        assert raw[size:] == b"\xa5" * (56 - size), size
        assert raw[:size] == bytes(rt.TonemapParams(struct_size=size, op=0, exposure=1.0, auto_key=0.0, delta=1e-4, white=th.INF))[:size], size
    for size in (0, 4, 12, 20, 41, 48):
        buf = (C.c_uint8 * 56)(*([0xA5] * 56))
        assert lib.rt_tonemap_params_init_sized(buf, size) == -1, size
        assert "struct_size" in lib.rt_last_error().decode()
        assert bytes(buf) == b"\xa5" * 56
    assert lib.rt_tonemap_params_init_sized(None, 40) == -1
    with pytest.raises(TypeError):
        rt.tonemap_params(gamma=2.2)
    assert rt.tonemap_params(op="aces").op == 2
    with pytest.raises(rt.RtError):
        rt.tonemap_params(op="filmic")


def test_the_workspace_is_refused_for_refused_sizes_and_is_monotone(rt):
    lib = rt.amd_lib()
    sizes = [(1, 1), (255, 1), (256, 1), (257, 1), (17, 9), (70, 37), (256, 256), (257, 255), (65537, 1), (1200, 800), (1 << 13, 1 << 13), ((1 << 27) - 1, 1)]
    sizes.sort(key=lambda s: s[0] * s[1])
    got = [lib.rt_tonemap_workspace_bytes(w, h) for w, h in sizes]
    assert all(b > 0 for b in got)
    assert got == sorted(got), "more pixels never need less"
    for (w, h), b in zip(sizes, got):
        n, entries = w * h, 0
        while True:
            n = -(-n // 256)
            entries += n
            if n == 1:
                break
        assert b == 32 + 16 * entries, (w, h)
        assert b % 16 == 0
        assert lib.rt_tonemap_workspace_bytes(h, w) == b, "a function of w * h"
    assert got[0] == 32 + 16 and lib.rt_tonemap_workspace_bytes(257, 1) == 32 + 16 * 3
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 14, 1 << 13), (1 << 27, 1)):
        assert lib.rt_tonemap_workspace_bytes(w, h) == -1
        with pytest.raises(rt.RtError):
            rt.tonemap_workspace_bytes(w, h)


def _tonemap(rt, *, w=6, h=4, v=True, spp=8, spp_map=False, params=None, rgb=True, rgba=True, ws=True, alias=None, misalign=False, ws_misalign=False):
    """One call of rt_tonemap_device on HOST buffers: only argument checks can answer (the first thing past them asks the HIP runtime
    which device owns an output, and host memory has none)."""
    lib = rt.amd_lib()
    n = w * h if w > 0 and h > 0 else 1
    V = (C.c_double * (3 * n))()
    N = (C.c_int32 * n)()
    B3 = (C.c_uint8 * (3 * n))()
    B4 = (C.c_uint8 * (4 * n + 4))()
    W = (C.c_uint8 * (64 * n + 64))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    rgb_ptr = C.addressof(B3)
    rgba_ptr = (C.addressof(B4) + 3) // 4 * 4 + (1 if misalign else 0)
    if alias == "rgb8":
        rgb_ptr = C.addressof(V) + 8 * (3 * n - 1)   # the last double of the values
    elif alias == "rgba8":
        rgba_ptr = C.addressof(V)
    rc = lib.rt_tonemap_device(w, h, C.addressof(V) if v else None, spp, C.addressof(N) if spp_map else None,
                               C.byref(params) if params is not None else None, rgb_ptr if rgb else None, rgba_ptr if rgba else None,
                               ws_ptr if ws else None, None)
    return rc, lib.rt_last_error().decode()


def test_every_invalid_tonemap_argument_is_named_without_a_device(rt):
    P = rt.TonemapParams
    nan, inf = float("nan"), float("inf")
    auto = rt.tonemap_params(auto_key=0.18)
    cases = [
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(v=False), "d_values is null"),
        (dict(rgb=False, rgba=False), "both null"),
        (dict(spp=0), "spp"), (dict(spp=-4), "spp"), (dict(spp=0, spp_map=True), "spp"),
        (dict(params=P(struct_size=12)), "struct_size"), (dict(params=P(struct_size=48)), "struct_size"), (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=rt.tonemap_params(op=3)), "op"), (dict(params=rt.tonemap_params(op=-1)), "op"),
        (dict(params=rt.tonemap_params(exposure=0.0)), "exposure"), (dict(params=rt.tonemap_params(exposure=-1.0)), "exposure"),
        (dict(params=rt.tonemap_params(exposure=nan)), "exposure"), (dict(params=rt.tonemap_params(exposure=inf)), "exposure"),
        (dict(params=rt.tonemap_params(delta=0.0)), "delta"), (dict(params=rt.tonemap_params(delta=nan)), "delta"),
        (dict(params=rt.tonemap_params(delta=inf)), "delta"),
        (dict(params=rt.tonemap_params(auto_key=-0.18)), "auto_key"), (dict(params=rt.tonemap_params(auto_key=nan)), "auto_key"),
        (dict(params=rt.tonemap_params(auto_key=inf)), "auto_key"),
        (dict(params=rt.tonemap_params(white=0.0)), "white"), (dict(params=rt.tonemap_params(white=-4.0)), "white"),
        (dict(params=rt.tonemap_params(white=nan)), "white"),
        (dict(params=auto, ws=False), "d_workspace"), (dict(params=auto, ws_misalign=True), "d_workspace"),
        (dict(misalign=True), "d_rgba8"),
        (dict(alias="rgb8"), "overlap"), (dict(alias="rgba8"), "overlap"),
    ]
    for kw, field in cases:
        rc, msg = _tonemap(rt, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith("rt_tonemap_device: "), (kw, msg)
    # the header's order: of two bad arguments the earlier one is named
    assert "d_values" in _tonemap(rt, v=False, spp=0)[1]
    assert "spp" in _tonemap(rt, spp=0, params=rt.tonemap_params(op=9))[1]
    assert "op" in _tonemap(rt, params=rt.tonemap_params(op=9, white=0.0, auto_key=0.18), ws=False)[1]
    assert "d_workspace" in _tonemap(rt, params=auto, ws=False, misalign=True)[1]
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(rgb=False), dict(rgba=False), dict(spp=1, spp_map=True), dict(ws=False), dict(ws_misalign=True), dict(params=auto),
               dict(params=rt.tonemap_params(op=2, exposure=1e-300, white=inf)), dict(params=rt.tonemap_params(op=1, white=4.0, delta=1e-300)),
               dict(params=P(struct_size=8, op=2)), dict(params=P(struct_size=16, op=1, exposure=2.0))):
        rc, msg = _tonemap(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)
    # a shorter struct's missing fields are the defaults, not the bytes behind it: white = 0 beyond struct_size 32 is not looked at
    rc, msg = _tonemap(rt, params=P(struct_size=32, op=1, exposure=1.0, auto_key=0.0, delta=1e-4, white=0.0))
    assert "not a device pointer" in msg, msg


def test_every_invalid_log_average_argument_is_named_without_a_device(rt):
    lib = rt.amd_lib()
    n = 24
    V, O = (C.c_double * (3 * n))(), (C.c_double * 4)()
    W = (C.c_uint8 * 256)()
    ws = (C.addressof(W) + 15) // 16 * 16

    def call(*, w=6, h=4, v=True, spp=1, delta=1e-4, out=C.addressof(O), work=ws):
        rc = lib.rt_log_average_luminance_device(w, h, C.addressof(V) if v else None, spp, None, delta, out, work, None)
        return rc, lib.rt_last_error().decode()

    for kw, field in ((dict(w=0), "width"), (dict(h=0), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"), (dict(v=False), "d_values"),
                      (dict(out=None), "d_out4"), (dict(spp=0), "spp"), (dict(delta=0.0), "delta"), (dict(delta=float("nan")), "delta"),
                      (dict(delta=float("inf")), "delta"), (dict(work=None), "d_workspace"), (dict(work=ws + 8), "d_workspace"),
                      (dict(out=C.addressof(V) + 8), "overlap")):
        rc, msg = call(**kw)
        assert rc == -1 and field in msg and msg.startswith("rt_log_average_luminance_device: "), (kw, rc, msg)
    rc, msg = call()
    assert rc != 0 and "not a device pointer" in msg
