"""The frame-metrics C ABI without a GPU: the symbols and their Rust declarations, the layout and the sized initialisers of the two params
structs, the workspace size, and every invalid argument of rt_frame_error_device and rt_frame_noise_device (checked before any device
work, in the header's order, the field named)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

import metrics_helpers as mh

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_frame_error_params_init_sized", "rt_frame_noise_params_init_sized", "rt_metrics_workspace_bytes", "rt_frame_error_device",
           "rt_frame_noise_device")
HOST_SYMBOLS = ("rth_frame_error", "rth_frame_noise", "rth_read_pfm")


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
    assert "pub struct rt_frame_error_params" in text and "pub struct rt_frame_noise_params" in text
    assert "frame metrics (opt-in; nothing above changes)" in header
    host_header = (ROOT / "include" / "rt_host.h").read_text()
    host = rt.host_lib()
    for fn in HOST_SYMBOLS:
        assert getattr(host, fn) is not None
        assert fn in rt.RT_HOST_SYMBOLS and re.search(r"\bint " + fn + r"\(", host_header), fn
    for name in ("frame_error_params", "frame_error_device", "frame_error", "frame_error_host", "frame_noise_params", "frame_noise_device",
                 "frame_noise", "frame_noise_host", "metrics_workspace_bytes", "read_pfm"):
        assert callable(getattr(rt, name)), name
    assert callable(rt.DeviceScene.render_until)
    assert (rt.RT_METRICS_SUMS, rt.RT_METRICS_MEANS) == (0, 1)
    for name, value in (("SUMS", 0), ("MEANS", 1)):
        assert re.search(rf"#define RT_METRICS_{name} {value}\b", header)
    assert rt.FRAME_ERROR_FIELDS == mh.ERROR_FIELDS and rt.FRAME_NOISE_FIELDS == mh.NOISE_FIELDS


@pytest.mark.parametrize("c_name,cls_name,size", [("rt_frame_error_params", "FrameErrorParams", 24), ("rt_frame_noise_params", "FrameNoiseParams", 16)])
def test_the_params_have_gccs_layout_and_their_rust_fields(rt, tmp_path, c_name, cls_name, size):
    cls = getattr(rt, cls_name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){", f'printf("size %zu\\n", sizeof({c_name}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({c_name}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) == size
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname
    text = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"pub struct " + c_name + r"\s*\{(.*?)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in cls._fields_]


def test_init_sized_writes_the_defaults_into_struct_size_bytes_only(rt):
    lib = rt.amd_lib()
    e, n = rt.frame_error_params(), rt.frame_noise_params()
    assert (e.struct_size, e.eps, e.peak) == (24, 1e-2, 1.0) and mh.ERROR_DEFAULTS == dict(eps=e.eps, peak=e.peak)
    assert (n.struct_size, n.eps) == (16, 1e-2) and mh.NOISE_DEFAULTS == dict(eps=n.eps)
    for init, full, good in ((lib.rt_frame_error_params_init_sized, rt.FrameErrorParams(eps=1e-2, peak=1.0), (8, 16, 24)),
                             (lib.rt_frame_noise_params_init_sized, rt.FrameNoiseParams(eps=1e-2), (8, 16))):
        for size in good:
            buf = (C.c_uint8 * 40)(*([0xA5] * 40))
            assert init(buf, size) == 0
            raw = bytes(buf)
            assert raw[size:] == b"\xa5" * (40 - size), size
            full.struct_size = size
            assert raw[:size] == bytes(full)[:size], size
        for size in (0, 4, 12, 20, good[-1] + 1, good[-1] + 8):
            buf = (C.c_uint8 * 40)(*([0xA5] * 40))
            assert init(buf, size) == -1, size
            assert "struct_size" in lib.rt_last_error().decode()
            assert bytes(buf) == b"\xa5" * 40
        assert init(None, 16) == -1
    with pytest.raises(TypeError):
        rt.frame_error_params(gamma=2.2)
    with pytest.raises(TypeError):
        rt.frame_noise_params(peak=1.0)


def test_the_workspace_is_refused_for_refused_sizes_and_is_monotone(rt):
    lib = rt.amd_lib()
    sizes = mh.SIZES + [(17, 9), (65537, 1), (1200, 800), (1 << 13, 1 << 13), ((1 << 27) - 1, 1)]
    sizes.sort(key=lambda s: s[0] * s[1])
    got = [lib.rt_metrics_workspace_bytes(w, h) for w, h in sizes]
    assert got == sorted(got), "more pixels never need less"
    for (w, h), b in zip(sizes, got):
        n, entries = w * h, 0
        while True:
            n = -(-n // 256)
            entries += n
            if n == 1:
                break
        assert b == 48 * entries and b % 16 == 0, (w, h)
        assert lib.rt_metrics_workspace_bytes(h, w) == b, "a function of w * h"
    assert lib.rt_metrics_workspace_bytes(1, 1) == 48 and lib.rt_metrics_workspace_bytes(257, 1) == 48 * 3
    assert lib.rt_metrics_workspace_bytes(257, 256) == 48 * (257 + 2 + 1)
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 14, 1 << 13), (1 << 27, 1)):
        assert lib.rt_metrics_workspace_bytes(w, h) == -1
        with pytest.raises(rt.RtError):
            rt.metrics_workspace_bytes(w, h)


class _Buffers:
    """HOST buffers for one call: only argument checks can answer (the first thing past them asks the HIP runtime which device owns the
    output, and host memory has none)."""

    def __init__(self, n=24):
        self.V, self.R = (C.c_double * (3 * n))(), (C.c_double * (3 * n))()
        self.N = (C.c_int32 * n)()
        self.O = (C.c_double * 8)()
        self.W = (C.c_uint8 * 4096)()
        self.ws = (C.addressof(self.W) + 15) // 16 * 16


def _error(rt, *, w=6, h=4, v=True, spp=1, spp_map=False, r=True, ref_spp=1, params=None, out="own", ws="own"):
    lib, b = rt.amd_lib(), _Buffers()
    out_ptr = {"own": C.addressof(b.O), None: None, "values": C.addressof(b.V) + 8, "ref": C.addressof(b.R) + 8 * (3 * 24 - 8)}[out]   # (the last eight doubles of the reference: inside it, so no other buffer is met)
    ws_ptr = {"own": b.ws, None: None, "misaligned": b.ws + 8}[ws]
    rc = lib.rt_frame_error_device(w, h, C.addressof(b.V) if v else None, spp, C.addressof(b.N) if spp_map else None, C.addressof(b.R) if r else None,
                                   ref_spp, C.byref(params) if params is not None else None, out_ptr, ws_ptr, None)
    return rc, lib.rt_last_error().decode()


def _noise(rt, *, w=6, h=4, form=0, a=True, b=True, n=4, spp_map=False, params=None, out="own", ws="own"):
    lib, bf = rt.amd_lib(), _Buffers()
    out_ptr = {"own": C.addressof(bf.O), None: None, "a": C.addressof(bf.V), "b": C.addressof(bf.R) + 8 * (3 * 24 - 4)}[out]   # (the last four doubles of d_b: inside it)
    ws_ptr = {"own": bf.ws, None: None, "misaligned": bf.ws + 8}[ws]
    rc = lib.rt_frame_noise_device(w, h, form, C.addressof(bf.V) if a else None, C.addressof(bf.R) if b else None, n, C.addressof(bf.N) if spp_map else None,
                                   C.byref(params) if params is not None else None, out_ptr, ws_ptr, None)
    return rc, lib.rt_last_error().decode()


def test_every_invalid_frame_error_argument_is_named_without_a_device(rt):
    P = rt.FrameErrorParams
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(v=False), "d_values is null"), (dict(r=False), "d_ref is null"), (dict(out=None), "d_out8 is null"),
        (dict(spp=0), "spp"), (dict(spp=0, spp_map=True), "spp"), (dict(ref_spp=0), "ref_spp"), (dict(ref_spp=-2), "ref_spp"),
        (dict(params=P(struct_size=12)), "struct_size"), (dict(params=P(struct_size=32)), "struct_size"), (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=rt.frame_error_params(eps=0.0)), "eps"), (dict(params=rt.frame_error_params(eps=-1.0)), "eps"),
        (dict(params=rt.frame_error_params(eps=nan)), "eps"), (dict(params=rt.frame_error_params(eps=inf)), "eps"),
        (dict(params=rt.frame_error_params(peak=0.0)), "peak"), (dict(params=rt.frame_error_params(peak=nan)), "peak"),
        (dict(params=rt.frame_error_params(peak=inf)), "peak"),
        (dict(ws=None), "d_workspace is null"), (dict(ws="misaligned"), "16-byte aligned"),
        (dict(out="values"), "overlap d_values"), (dict(out="ref"), "overlap d_ref"),
    ]
    for kw, field in cases:
        rc, msg = _error(rt, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith("rt_frame_error_device: "), (kw, msg)
    # the header's order: of two bad arguments the earlier one is named
    assert "width" in _error(rt, w=0, v=False)[1]
    assert "d_values" in _error(rt, v=False, r=False)[1]
    assert "d_ref" in _error(rt, r=False, out=None)[1]
    assert "d_out8" in _error(rt, out=None, spp=0)[1]
    assert "spp must" in _error(rt, spp=0, ref_spp=0)[1]
    assert "ref_spp" in _error(rt, ref_spp=0, params=P(struct_size=12))[1]
    assert "struct_size" in _error(rt, params=P(struct_size=12, eps=0.0), ws=None)[1]
    assert "eps" in _error(rt, params=rt.frame_error_params(eps=0.0, peak=0.0))[1]
    assert "peak" in _error(rt, params=rt.frame_error_params(peak=0.0), ws=None)[1]
    assert "d_workspace" in _error(rt, ws=None, out="values")[1]
    # what is fine gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(spp=12, ref_spp=48), dict(spp=1, spp_map=True), dict(params=rt.frame_error_params(eps=1e-300, peak=1e300)),
               dict(params=P(struct_size=8)), dict(params=P(struct_size=16, eps=0.5, peak=0.0))):
        rc, msg = _error(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)


def test_every_invalid_frame_noise_argument_is_named_without_a_device(rt):
    P = rt.FrameNoiseParams
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(w=0), "width"), (dict(h=0), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(a=False), "d_a is null"), (dict(b=False), "d_b is null"), (dict(out=None), "d_out4 is null"),
        (dict(n=0), "n must"), (dict(n=-1, spp_map=True), "n must"),
        (dict(params=P(struct_size=12)), "struct_size"), (dict(params=P(struct_size=24)), "struct_size"),
        (dict(form=2), "form"), (dict(form=-1), "form"), (dict(form=1, spp_map=True), "RT_METRICS_MEANS"),
        (dict(params=rt.frame_noise_params(eps=0.0)), "eps"), (dict(params=rt.frame_noise_params(eps=nan)), "eps"),
        (dict(params=rt.frame_noise_params(eps=inf)), "eps"),
        (dict(ws=None), "d_workspace is null"), (dict(ws="misaligned"), "16-byte aligned"),
        (dict(out="a"), "overlap d_a"), (dict(out="b"), "overlap d_b"),
    ]
    for kw, field in cases:
        rc, msg = _noise(rt, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith("rt_frame_noise_device: "), (kw, msg)
    assert "d_a" in _noise(rt, a=False, b=False)[1]
    assert "d_out4" in _noise(rt, out=None, n=0)[1]
    assert "n must" in _noise(rt, n=0, params=P(struct_size=12))[1]
    assert "struct_size" in _noise(rt, params=P(struct_size=12), form=7)[1]
    assert "form" in _noise(rt, form=7, params=rt.frame_noise_params(eps=0.0))[1]
    assert "eps" in _noise(rt, params=rt.frame_noise_params(eps=0.0), ws=None)[1]
    assert "d_workspace" in _noise(rt, ws="misaligned", out="a")[1]
    for kw in (dict(), dict(form=1), dict(n=1), dict(spp_map=True), dict(params=P(struct_size=8)), dict(params=rt.frame_noise_params(eps=1e-300))):
        rc, msg = _noise(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)


def test_the_host_mirrors_refuse_the_same_things_with_the_same_words(rt):
    import numpy as np
    frame = np.ones((4, 6, 3))
    for kw, field in ((dict(spp=0), "spp must"), (dict(ref_spp=0), "ref_spp"), (dict(eps=0.0), "eps"), (dict(peak=float("nan")), "peak")):
        args = dict(spp=1, ref_spp=1) | kw
        with pytest.raises(rt.RtError) as e:
            rt.frame_error_host(frame, args.pop("spp"), frame, args.pop("ref_spp"), **args)
        assert field in str(e.value) and str(e.value).startswith("rth_frame_error: ")
    for kw, field in ((dict(n=0), "n must"), (dict(form=5), "form"), (dict(form="means", spp_map=np.ones((4, 6), dtype=np.int32)), "RT_METRICS_MEANS"),
                      (dict(eps=-1.0), "eps")):
        args = dict(n=4) | kw
        with pytest.raises(rt.RtError) as e:
            rt.frame_noise_host(frame, frame, args.pop("n"), **args)
        assert field in str(e.value) and str(e.value).startswith("rth_frame_noise: ")
    with pytest.raises(rt.RtError):
        rt.frame_error_host(frame, 1, np.ones((4, 5, 3)), 1)
    with pytest.raises(rt.RtError):
        rt.frame_noise(frame, frame, 4, form="variances")
