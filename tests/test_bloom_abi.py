"""Bloom's C ABI without a GPU: the symbols and their Rust declarations, the layout and the sized initialiser of rt_bloom_params, the
workspace size, and every invalid argument of rt_bloom_device in the header's order (checked before any device work, the field named)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

import bloom_helpers as bh

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_bloom_params_init_sized", "rt_bloom_workspace_bytes", "rt_bloom_device")


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
    assert "pub struct rt_bloom_params" in text
    assert "bloom (opt-in; nothing above changes)" in header
    assert header.index("bloom (opt-in; nothing above changes)") < header.index("tone mapping (opt-in; nothing above changes)"), "bloom runs before the tone mapper"
    assert re.search(r"#define RT_ABI_VERSION 2\b", header)
    host_header = (ROOT / "include" / "rt_host.h").read_text()
    host_exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_host.so")], check=True, capture_output=True, text=True).stdout
    assert "rth_bloom" in rt.RT_HOST_SYMBOLS and re.search(r"\bint rth_bloom\(", host_header) and re.search(r" T rth_bloom$", host_exported, flags=re.M)
    for name in ("bloom_params", "bloom_workspace_bytes", "bloom_device", "bloom", "bloom_host"):
        assert callable(getattr(rt, name)), name


def test_rt_bloom_params_has_gccs_layout_and_its_rust_fields(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){", 'printf("size %zu\\n", sizeof(rt_bloom_params));']
    for fname, _ in rt.BloomParams._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rt_bloom_params, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(rt.BloomParams) == 24
    for fname, _ in rt.BloomParams._fields_:
        assert int(got[fname]) == getattr(rt.BloomParams, fname).offset, fname
    text = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"pub struct rt_bloom_params\s*\{(.*?)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in rt.BloomParams._fields_]


def test_init_sized_writes_the_defaults_into_struct_size_bytes_only(rt):
    lib = rt.amd_lib()
    b = rt.bloom_params()
    assert (b.struct_size, b.levels, b.threshold, b.strength) == (24, 5, 1.0, 0.25)
    assert bh.DEFAULTS == dict(levels=b.levels, threshold=b.threshold, strength=b.strength)
    for size in (8, 16, 24):
        buf = (C.c_uint8 * 40)(*([0xA5] * 40))
        assert lib.rt_bloom_params_init_sized(buf, size) == 0
        raw = bytes(buf)
        assert raw[size:] == b"\xa5" * (40 - size), size
        assert raw[:size] == bytes(rt.BloomParams(struct_size=size, levels=5, threshold=1.0, strength=0.25))[:size], size
    for size in (0, 4, 12, 20, 25, 32):
        buf = (C.c_uint8 * 40)(*([0xA5] * 40))
        assert lib.rt_bloom_params_init_sized(buf, size) == -1, size
        assert "struct_size" in lib.rt_last_error().decode()
        assert bytes(buf) == b"\xa5" * 40
    assert lib.rt_bloom_params_init_sized(None, 24) == -1
    with pytest.raises(TypeError):
        rt.bloom_params(radius=3)


def test_the_workspace_is_three_regions_of_the_frame(rt):
    lib = rt.amd_lib()
    for w, h in ((1, 1), (1, 7), (5, 3), (17, 9), (64, 16), (65, 17), (1200, 800), (1 << 13, 1 << 13), ((1 << 27) - 1, 1)):
        region = (w * h * 24 + 15) // 16 * 16
        assert lib.rt_bloom_workspace_bytes(w, h) == 3 * region == rt.bloom_workspace_bytes(w, h), (w, h)
        assert lib.rt_bloom_workspace_bytes(h, w) == 3 * region, "a function of w * h"
    assert lib.rt_bloom_workspace_bytes(1, 1) == 96
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 14, 1 << 13), (1 << 27, 1)):
        assert lib.rt_bloom_workspace_bytes(w, h) == -1
        with pytest.raises(rt.RtError):
            rt.bloom_workspace_bytes(w, h)


def _bloom(rt, *, w=6, h=4, v=True, out=True, ws=True, spp=8, spp_map=False, params=None, ws_misalign=False, alias=False):
    """One call of rt_bloom_device on HOST buffers: only argument checks can answer (the first thing past them asks the HIP runtime
    which device owns the output, and host memory has none)."""
    lib = rt.amd_lib()
    n = w * h if w > 0 and h > 0 and w * h < 1 << 20 else 1
    V = (C.c_double * (3 * n))()
    O = (C.c_double * (3 * n))()
    N = (C.c_int32 * n)()
    W = (C.c_uint8 * (72 * n + 64))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    out_ptr = C.addressof(V) + 8 * (3 * n - 1) if alias else C.addressof(O)   # alias: the last double of the values
    rc = lib.rt_bloom_device(w, h, C.addressof(V) if v else None, spp, C.addressof(N) if spp_map else None,
                             C.byref(params) if params is not None else None, out_ptr if out else None, ws_ptr if ws else None, None)
    return rc, lib.rt_last_error().decode()


def test_every_invalid_argument_is_named_without_a_device_in_the_headers_order(rt):
    P = rt.BloomParams
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(v=False), "d_values is null"), (dict(out=False), "d_mean_out is null"), (dict(ws=False), "d_workspace is null"),
        (dict(spp=0), "spp"), (dict(spp=-4), "spp"), (dict(spp=0, spp_map=True), "spp"),
        (dict(params=P(struct_size=12)), "struct_size"), (dict(params=P(struct_size=32)), "struct_size"), (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=rt.bloom_params(levels=0)), "levels"), (dict(params=rt.bloom_params(levels=9)), "levels"), (dict(params=rt.bloom_params(levels=-1)), "levels"),
        (dict(params=rt.bloom_params(threshold=-1.0)), "threshold"), (dict(params=rt.bloom_params(threshold=nan)), "threshold"),
        (dict(params=rt.bloom_params(threshold=inf)), "threshold"),
        (dict(params=rt.bloom_params(strength=-0.5)), "strength"), (dict(params=rt.bloom_params(strength=nan)), "strength"),
        (dict(params=rt.bloom_params(strength=inf)), "strength"),
        (dict(ws_misalign=True), "16-byte aligned"),
        (dict(alias=True), "overlap"),
    ]
    for kw, field in cases:
        rc, msg = _bloom(rt, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith("rt_bloom_device: "), (kw, msg)
    # the header's order: of two bad arguments the earlier one is named — each entry is bad in its own way and in every later way
    order = [(dict(w=0), "width"), (dict(v=False), "d_values"), (dict(out=False), "d_mean_out"), (dict(ws=False), "d_workspace is null"),
             (dict(spp=0), "spp"), (dict(params=P(struct_size=12, levels=0)), "struct_size"), (dict(levels=0), "levels"),
             (dict(threshold=-1.0), "threshold"), (dict(strength=-1.0), "strength"), (dict(ws_misalign=True), "aligned"), (dict(alias=True), "overlap")]
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kw, fields = {}, {}
            for extra, _ in (order[a], order[b]):
                for key, value in extra.items():
                    (fields if key in ("levels", "threshold", "strength") else kw)[key] = value
            if "ws" in kw and "ws_misalign" in kw:
                continue   # (a null workspace has no alignment)
            if fields:
                if "params" in kw:
                    continue   # (an unknown struct's fields are not looked at)
                kw["params"] = rt.bloom_params(**fields)
            rc, msg = _bloom(rt, **kw)
            assert rc == -1 and order[a][1] in msg, (order[a], order[b], msg)
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(spp=1, spp_map=True), dict(params=rt.bloom_params(levels=1, threshold=0.0, strength=0.0)), dict(params=rt.bloom_params(levels=8)),
               dict(params=P(struct_size=8, levels=2)), dict(params=P(struct_size=16, levels=3, threshold=2.0))):
        rc, msg = _bloom(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)
    # a shorter struct's missing fields are the defaults, not the bytes behind it: strength = -1 beyond struct_size 16 is not looked at
    rc, msg = _bloom(rt, params=P(struct_size=16, levels=5, threshold=1.0, strength=-1.0))
    assert "not a device pointer" in msg, msg


def test_the_host_mirror_refuses_the_same_things_with_the_same_words(rt):
    lib, host = rt.amd_lib(), rt.host_lib()
    n = 24
    V, O = (C.c_double * (3 * n))(), (C.c_double * (3 * n))()
    W = (C.c_uint8 * (72 * n + 16))()
    ws = (C.addressof(W) + 15) // 16 * 16
    P = rt.BloomParams
    for kw in (dict(w=0), dict(h=0), dict(w=1 << 14, h=1 << 13), dict(spp=0), dict(params=P(struct_size=12)), dict(params=rt.bloom_params(levels=9)),
               dict(params=rt.bloom_params(threshold=-1.0)), dict(params=rt.bloom_params(strength=float("nan"))), dict(out=C.addressof(V) + 8)):
        a = dict(w=6, h=4, spp=1, params=None, out=C.addressof(O))
        a.update(kw)
        p = C.byref(a["params"]) if a["params"] is not None else None
        assert lib.rt_bloom_device(a["w"], a["h"], C.addressof(V), a["spp"], None, p, a["out"], ws, None) == -1, kw
        assert host.rth_bloom(a["w"], a["h"], C.addressof(V), a["spp"], None, p, a["out"]) == -1, kw
        dev, mirror = lib.rt_last_error().decode(), host.rth_last_error().decode()
        assert dev.startswith("rt_bloom_device: ") and mirror.startswith("rth_bloom: ")
        tail = dev[len("rt_bloom_device: "):]
        assert mirror[len("rth_bloom: "):] == tail.replace("d_mean_out", "out_mean").replace("d_values", "values"), (kw, dev, mirror)
    for name, args in (("values is null", (6, 4, None, 1, None, None, C.addressof(O))), ("out_mean is null", (6, 4, C.addressof(V), 1, None, None, None))):
        assert host.rth_bloom(*args) == -1 and host.rth_last_error().decode() == "rth_bloom: " + name
