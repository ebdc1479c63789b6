"""Adaptive sampling's C ABI without a GPU: struct layouts against gcc, the Rust binding in INTEGRATION.md, the sized init's
defaults and guard, every invalid argument (checked before the scene handle and the device), and the command line's refusals."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _structs(rt):
    return {"rt_adaptive_params": rt.AdaptiveParams, "rt_adaptive_result": rt.AdaptiveResult}


def test_adaptive_structs_match_the_c_layout(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){"]
    for cname, cls in _structs(rt).items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["rt_adaptive_params"]) == 32 and int(got["rt_adaptive_result"]) == 16
    for cname, cls in _structs(rt).items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_integration_md_declares_the_adaptive_structs_in_order(rt):
    text = (ROOT / "INTEGRATION.md").read_text()
    rust = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", text), flags=re.S)
    for cname, cls in _structs(rt).items():
        m = re.search(r"pub struct " + cname + r"\s*\{(.*?)\}", rust, flags=re.S)
        assert m, f"INTEGRATION.md declares no struct {cname}"
        assert re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in cls._fields_], cname
    for fn in ("rt_adaptive_params_init_sized", "rt_render_pixels_device", "rt_render_adaptive", "rt_render_adaptive_device",
               "rt_resolve_rgb8_spp_device"):
        assert f"pub fn {fn}(" in text, fn


def test_sized_init_fills_the_defaults_and_writes_nothing_beyond_struct_size(rt):
    lib = rt.amd_lib()
    a = rt.AdaptiveParams()
    assert lib.rt_adaptive_params_init_sized(C.addressof(a), C.sizeof(a)) == 0
    assert (a.struct_size, a.min_spp, a.batch_spp, a.rel_threshold, a.abs_threshold) == (32, 16, 16, 0.02, 1e-3)
    # a caller whose struct is 16 bytes long: the 16 bytes behind it (its guard) stay as they were
    buf = (C.c_uint8 * 32)()
    C.memset(buf, 0xAB, 32)
    assert lib.rt_adaptive_params_init_sized(C.addressof(buf), 16) == 0
    short = rt.AdaptiveParams.from_buffer_copy(bytes(buf))
    assert (short.struct_size, short.min_spp, short.batch_spp) == (16, 16, 16)
    assert bytes(buf)[16:] == b"\xab" * 16, "the sized init wrote past the caller's struct"
    for bad in (0, 4, 6, 33, 64):
        assert lib.rt_adaptive_params_init_sized(C.addressof(a), bad) == -1, bad
    assert lib.rt_adaptive_params_init_sized(None, 32) == -1


def _call(rt, *, scene=None, params=None, adaptive=None, camera=True, sums=True, spp=True, result=True, device=False):
    """One call of rt_render_adaptive (or its device form) with a NULL scene: only argument checks can answer."""
    lib = rt.amd_lib()
    hs = rt.HostScene(6, width=16, spp=8, depth=4)
    cam = hs.camera
    p = params if params is not None else rt.render_params(seed=1)
    a = adaptive if adaptive is not None else rt.adaptive_params()
    n = cam.image_width * cam.image_height
    out_sum = (C.c_double * (3 * n))()
    out_spp = (C.c_int32 * n)()
    res = rt.AdaptiveResult()
    args = [scene, C.byref(cam) if camera else None, C.byref(p) if p is not False else None,
            C.byref(a) if a is not False else None, C.addressof(out_sum) if sums else None,
            C.addressof(out_spp) if spp else None, None]
    if device:
        rc = lib.rt_render_adaptive_device(*args, None, C.byref(res) if result else None)
    else:
        rc = lib.rt_render_adaptive(*args, C.byref(res) if result else None)
    return rc, lib.rt_last_error().decode()


@pytest.mark.parametrize("device", [False, True])
def test_every_invalid_adaptive_argument_is_named_before_the_scene_is_looked_at(rt, device):
    cases = [
        (dict(adaptive=rt.adaptive_params(min_spp=1)), "min_spp"),
        (dict(adaptive=rt.adaptive_params(min_spp=0)), "min_spp"),
        (dict(adaptive=rt.adaptive_params(min_spp=-3)), "min_spp"),
        (dict(adaptive=rt.adaptive_params(batch_spp=0)), "batch_spp"),
        (dict(adaptive=rt.adaptive_params(rel_threshold=-0.1)), "rel_threshold"),
        (dict(adaptive=rt.adaptive_params(rel_threshold=math.nan)), "rel_threshold"),
        (dict(adaptive=rt.adaptive_params(abs_threshold=-1e-9)), "abs_threshold"),
        (dict(adaptive=rt.adaptive_params(abs_threshold=math.nan)), "abs_threshold"),
        (dict(adaptive=rt.adaptive_params(struct_size=4)), "struct_size"),
        (dict(adaptive=rt.adaptive_params(struct_size=4096)), "struct_size"),
        (dict(params=rt.render_params(shard_count=2)), "shard_count"),
        (dict(params=rt.render_params(sample_begin=1)), "sample_begin"),
        (dict(params=rt.render_params(accumulate=True)), "accumulate"),
        (dict(adaptive=False), "adaptive"),
        (dict(camera=False), "camera"),
        (dict(params=False), "params"),
        (dict(sums=False), "d_sum" if device else "out_rgb_sum"),
        (dict(spp=False), "d_spp" if device else "out_spp"),
        (dict(result=False), "out_result"),
        (dict(), "scene"),  # every other argument is fine: the null scene is what is left
    ]
    for kw, field in cases:
        rc, msg = _call(rt, device=device, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg, (kw, msg)


def test_min_spp_is_clipped_to_max_spp(rt):
    # max_spp 1: min_spp is clipped to 1, which is then allowed (the rule is never evaluated below 2 samples)
    rc, msg = _call(rt, params=rt.render_params(sample_end=1), adaptive=rt.adaptive_params(min_spp=64))
    assert rc == -1 and "scene" in msg, msg
    # max_spp 8: min_spp 64 is clipped to 8
    rc, msg = _call(rt, adaptive=rt.adaptive_params(min_spp=64))
    assert rc == -1 and "scene" in msg, msg


def test_render_pixels_device_rejects_bad_arguments_without_a_gpu(rt):
    lib = rt.amd_lib()
    hs = rt.HostScene(6, width=16, spp=8, depth=4)
    p = rt.render_params()
    assert lib.rt_render_pixels_device(None, C.byref(hs.camera), C.byref(p), None, 4, None, None, None) == -1
    assert b"null" in lib.rt_last_error()


def test_rtrace_refuses_adaptive_with_several_gpus_or_progressive(rt, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "--adaptive", "0.05", "-o", str(tmp_path / "x")]
    for extra in (["--gpus", "2"], ["--progressive", "2"]):
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert "--adaptive" in r.stderr
    assert not (tmp_path / "x.png").exists()
