"""Robust frames' C ABI without a GPU: the symbols and their Rust declarations, the layout and the sized initialiser of rt_robust_params,
and every invalid argument of rt_robust_device in the header's order (checked before any device work, the field named)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

import robust_helpers as rh

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_robust_params_init_sized", "rt_robust_device")


def test_the_symbols_are_exported_declared_and_bound(rt):
    lib = rt.amd_lib()
    header = (ROOT / "include" / "rt_amd.h").read_text()
    text = (ROOT / "INTEGRATION.md").read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_amd.so")], check=True, capture_output=True, text=True).stdout
    for fn in SYMBOLS:
        assert getattr(lib, fn) is not None
        assert fn in rt.RT_AMD_SYMBOLS, fn
        assert re.search(r"\bint " + fn + r"\(", header), fn
        assert f"pub fn {fn}(" in text, fn
        assert re.search(r" T " + fn + r"$", exported, flags=re.M), fn
    assert "pub struct rt_robust_params" in text
    assert "robust frames (opt-in; nothing above changes)" in header
    for name, value in (("RT_ROBUST_MAX_BLOCKS", 32), ("RT_ROBUST_MEAN", 0), ("RT_ROBUST_TRIM", 1), ("RT_ROBUST_MEDIAN", 2), ("RT_ROBUST_GINI", 3)):
        assert re.search(rf"#define {name} {value}\b", header) and getattr(rt, name) == value, name
    assert (rh.MEAN, rh.TRIM, rh.MEDIAN, rh.GINI, rh.MAX_BLOCKS) == (0, 1, 2, 3, 32)
    assert re.search(r"#define RT_ABI_VERSION 2\b", header)
    assert "rt_debug_set_robust_form" in rt.RT_AMD_DEBUG_SYMBOLS and re.search(r" T rt_debug_set_robust_form$", exported, flags=re.M)
    assert re.search(r"\bint rt_debug_set_robust_form\(", (ROOT / "include" / "rt_amd_debug.h").read_text())
    host_header = (ROOT / "include" / "rt_host.h").read_text()
    host_exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_host.so")], check=True, capture_output=True, text=True).stdout
    assert "rth_robust" in rt.RT_HOST_SYMBOLS and re.search(r"\bint rth_robust\(", host_header) and re.search(r" T rth_robust$", host_exported, flags=re.M)
    for name in ("robust_params", "robust_device", "robust", "robust_host"):
        assert callable(getattr(rt, name)), name
    assert callable(rt.DeviceScene.render_robust)


def test_rt_robust_params_has_gccs_layout_and_its_rust_fields(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){", 'printf("size %zu\\n", sizeof(rt_robust_params));']
    for fname, _ in rt.RobustParams._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rt_robust_params, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(rt.RobustParams) == 24
    for fname, _ in rt.RobustParams._fields_:
        assert int(got[fname]) == getattr(rt.RobustParams, fname).offset, fname
    text = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"pub struct rt_robust_params\s*\{(.*?)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in rt.RobustParams._fields_]


def test_init_sized_writes_the_defaults_into_struct_size_bytes_only(rt):
    lib = rt.amd_lib()
    r = rt.robust_params()
    assert (r.struct_size, r.mode, r.trim, r.gain) == (24, rt.RT_ROBUST_GINI, 1, 1.0)
    assert rh.DEFAULTS == dict(mode=r.mode, trim=r.trim, gain=r.gain)
    for size in (8, 16, 24):
        buf = (C.c_uint8 * 40)(*([0xA5] * 40))
        assert lib.rt_robust_params_init_sized(buf, size) == 0
        raw = bytes(buf)
        assert raw[size:] == b"\xa5" * (40 - size), size
        assert raw[:size] == bytes(rt.RobustParams(struct_size=size, mode=3, trim=1, gain=1.0))[:size], size
    for size in (0, 4, 12, 20, 25, 32):
        buf = (C.c_uint8 * 40)(*([0xA5] * 40))
        assert lib.rt_robust_params_init_sized(buf, size) == -1, size
        assert "struct_size" in lib.rt_last_error().decode()
        assert bytes(buf) == b"\xa5" * 40
    assert lib.rt_robust_params_init_sized(None, 24) == -1
    with pytest.raises(TypeError):
        rt.robust_params(levels=3)
    assert rt.robust_params(mode="median").mode == rt.RT_ROBUST_MEDIAN
    with pytest.raises(rt.RtError):
        rt.robust_params(mode="mode")


def _robust(rt, *, w=6, h=4, blocks=3, stack=True, out=True, m2=True, spp=8, params=None, alias=None):
    """One call of rt_robust_device on HOST buffers: only argument checks can answer (the first thing past them asks the HIP runtime
    which device owns the output, and host memory has none)."""
    lib = rt.amd_lib()
    n = w * h if w > 0 and h > 0 and w * h < 1 << 20 else 1
    k = blocks if 1 <= blocks <= 32 else 1
    S = (C.c_double * (3 * n * k))()
    O = (C.c_double * (6 * n))()
    out_ptr, m2_ptr = C.addressof(O), C.addressof(O) + 24 * n
    if alias == "out_last_block":
        out_ptr = C.addressof(S) + 8 * (3 * n * k - 1)      # the last double of the last block
    elif alias == "m2_first_block":
        m2_ptr = C.addressof(S)
    elif alias == "m2_out":
        m2_ptr = out_ptr + 8 * (3 * n - 1)
    rc = lib.rt_robust_device(w, h, blocks, C.addressof(S) if stack else None, spp, C.byref(params) if params is not None else None,
                              out_ptr if out else None, m2_ptr if m2 else None, None)
    return rc, lib.rt_last_error().decode()


def test_every_invalid_argument_is_named_without_a_device_in_the_headers_order(rt):
    P = rt.RobustParams
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(blocks=0), "blocks"), (dict(blocks=33), "blocks"), (dict(blocks=-2), "blocks"),
        (dict(stack=False), "d_stack is null"), (dict(out=False), "d_mean_out is null"),
        (dict(spp=0), "spp"), (dict(spp=-4), "spp"),
        (dict(params=P(struct_size=12)), "struct_size"), (dict(params=P(struct_size=32)), "struct_size"), (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=rt.robust_params(mode=-1)), "mode"), (dict(params=rt.robust_params(mode=4)), "mode"),
        (dict(params=rt.robust_params(trim=-1)), "trim"),
        (dict(params=rt.robust_params(gain=0.0)), "gain"), (dict(params=rt.robust_params(gain=-1.0)), "gain"), (dict(params=rt.robust_params(gain=nan)), "gain"),
        (dict(params=rt.robust_params(gain=inf)), "gain"),
        (dict(alias="out_last_block"), "d_mean_out must not overlap d_stack"), (dict(alias="m2_first_block"), "d_m2_out must not overlap d_stack"),
        (dict(alias="m2_out"), "d_m2_out must not overlap d_mean_out"),
    ]
    for kw, field in cases:
        rc, msg = _robust(rt, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith("rt_robust_device: "), (kw, msg)
    # the header's order: of two bad arguments the earlier one is named — each entry is bad in its own way and in every later way
    order = [(dict(w=0), "width"), (dict(blocks=0), "blocks"), (dict(stack=False), "d_stack"), (dict(out=False), "d_mean_out is null"), (dict(spp=0), "spp"),
             (dict(params=P(struct_size=12, mode=9)), "struct_size"), (dict(mode=9), "mode"), (dict(trim=-1), "trim"), (dict(gain=-1.0), "gain"),
             (dict(alias="m2_out"), "overlap")]
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kw, fields = {}, {}
            for extra, _ in (order[a], order[b]):
                for key, value in extra.items():
                    (fields if key in ("mode", "trim", "gain") else kw)[key] = value
            if fields:
                if "params" in kw:
                    continue   # (an unknown struct's fields are not looked at)
                kw["params"] = rt.robust_params(**fields)
            rc, msg = _robust(rt, **kw)
            assert rc == -1 and order[a][1] in msg, (order[a], order[b], msg)
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(m2=False), dict(blocks=1, spp=1), dict(blocks=32), dict(params=rt.robust_params(mode=0, trim=99, gain=1e-300)),
               dict(params=P(struct_size=8, mode=2)), dict(params=P(struct_size=16, mode=1, trim=4))):
        rc, msg = _robust(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)
    # a shorter struct from an older caller keeps the defaults, not the bytes behind it: gain = -1 beyond struct_size 16 is not looked at
    rc, msg = _robust(rt, params=P(struct_size=16, mode=3, trim=1, gain=-1.0))
    assert "not a device pointer" in msg, msg
    rc, msg = _robust(rt, params=P(struct_size=8, mode=1, trim=-5))
    assert "not a device pointer" in msg, msg


def test_the_host_mirror_refuses_the_same_things_with_the_same_words(rt):
    lib, host = rt.amd_lib(), rt.host_lib()
    n = 24
    S, O = (C.c_double * (3 * n * 3))(), (C.c_double * (6 * n))()
    P = rt.RobustParams
    for kw in (dict(w=0), dict(h=0), dict(w=1 << 14, h=1 << 13), dict(blocks=0), dict(blocks=33), dict(spp=0), dict(params=P(struct_size=12)),
               dict(params=rt.robust_params(mode=4)), dict(params=rt.robust_params(trim=-1)), dict(params=rt.robust_params(gain=float("nan"))),
               dict(out=C.addressof(S) + 8 * (9 * n - 1)), dict(m2=C.addressof(S) + 8), dict(m2=C.addressof(O) + 8)):
        a = dict(w=6, h=4, blocks=3, spp=1, params=None, out=C.addressof(O), m2=C.addressof(O) + 24 * n)
        a.update(kw)
        p = C.byref(a["params"]) if a["params"] is not None else None
        assert lib.rt_robust_device(a["w"], a["h"], a["blocks"], C.addressof(S), a["spp"], p, a["out"], a["m2"], None) == -1, kw
        assert host.rth_robust(a["w"], a["h"], a["blocks"], C.addressof(S), a["spp"], p, a["out"], a["m2"]) == -1, kw
        dev, mirror = lib.rt_last_error().decode(), host.rth_last_error().decode()
        assert dev.startswith("rt_robust_device: ") and mirror.startswith("rth_robust: ")
        tail = dev[len("rt_robust_device: "):]
        assert mirror[len("rth_robust: "):] == tail.replace("d_mean_out", "out_mean").replace("d_m2_out", "out_m2").replace("d_stack", "stack"), (kw, dev, mirror)
    for name, args in (("stack is null", (6, 4, 3, None, 1, None, C.addressof(O), None)), ("out_mean is null", (6, 4, 3, C.addressof(S), 1, None, None, None))):
        assert host.rth_robust(*args) == -1 and host.rth_last_error().decode() == "rth_robust: " + name
