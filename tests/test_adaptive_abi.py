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


@pytest.mark.parametrize("device", [False, True])
def test_a_frame_of_2_to_the_27_pixels_is_refused_before_the_scene_is_looked_at(rt, device):
    lib = rt.amd_lib()
    hs = rt.HostScene(6, width=16, spp=8, depth=4)
    p, a, res = rt.render_params(seed=1), rt.adaptive_params(), rt.AdaptiveResult()
    one = (C.c_double * 3)()  # (never written: every call here ends in an argument check)
    for width, height, field in ((16384, 8192, "2^27"), (8192, 16384, "2^27"), (1 << 27, 1, "2^27"), (46341, 46341, "2^31"),
                                 (16384, 8191, "scene"), ((1 << 27) - 1, 1, "scene")):
        cam = rt.Camera.from_buffer_copy(hs.camera)
        cam.image_width, cam.image_height = width, height
        args = [None, C.byref(cam), C.byref(p), C.byref(a), C.addressof(one), C.addressof(one), None]
        rc = lib.rt_render_adaptive_device(*args, None, C.byref(res)) if device else lib.rt_render_adaptive(*args, C.byref(res))
        msg = lib.rt_last_error().decode()
        assert rc == -1 and field in msg, (width, height, rc, msg)


def test_the_exact_reciprocal_decode_of_a_list_entry_is_the_integer_division():
    """List mode finds an entry's row as trunc((e + 0.5) * (1 / w)) in f64 (rt_kernel.hip, LIST branch) for frames of fewer than 2^27
    pixels: the same operations in numpy against e // w — every entry within 3 of a row boundary (of every row, or of 2 million rows
    spread over the frame and its ends), and 4 million random entries, per width."""
    import numpy as np
    g = np.random.default_rng(1)
    limit = 1 << 27
    for w in (1, 3, 37, 1200, 4099, 8191, limit - 1):
        rows_all = limit // w + 1
        rows = np.arange(rows_all, dtype=np.int64) if rows_all <= (1 << 21) else np.unique(np.concatenate(
            [np.arange(1 << 19), rows_all - 1 - np.arange(1 << 19), g.integers(0, rows_all, 1 << 20)]))
        e = (rows[:, None] * w + np.arange(-3, 4)[None, :]).reshape(-1)
        e = np.concatenate([e, g.integers(0, limit, 1 << 22), [0, limit - 1]])
        e = e[(e >= 0) & (e < limit)]
        inv_w = 1.0 / np.float64(w)
        j = np.trunc((e.astype(np.float64) + 0.5) * inv_w).astype(np.int64)
        assert np.array_equal(j, e // w), (w, int((j != e // w).sum()))
        assert np.array_equal(e - j * w, e % w)


def test_the_constructed_rule_families_hold_both_verdicts():
    """The builders of tests/test_gpu_adaptive_step.py, run on the CPU under the numpy reference: a family that held one verdict only
    would prove nothing on the device.  Ties are ties (e2 == tol^2 exactly) with a neighbour on either side; at least 10 000 cases
    get another verdict from a fused multiply-add, in both directions."""
    import numpy as np
    import test_gpu_adaptive_step as t
    for name, S, Q, n, rel, abs_ in t.random_value_groups(count=20000):
        share = t.verdicts(S, Q, n, rel, abs_).mean()
        assert 0.2 < share < 0.8, (name, share)
    for name, S, Q, n, rel, abs_ in t.tie_groups():
        v = t.verdicts(S, Q, n, rel, abs_).reshape(3, 3)  # channel x (tie, above, below)
        assert (v == np.array([True, False, True])).all(), (name, v)
        m = S / float(n)
        var = (Q - S * m) / float(n - 1)
        tol = rel * (((m[:, 0] + m[:, 1]) + m[:, 2]) / 3.0) + abs_
        assert (var.max(axis=1)[0::3] / float(n) == (tol * tol)[0::3]).all(), name
    for family in (t.cancellation_groups, t.edge_groups):
        seen = set()
        for name, S, Q, n, rel, abs_ in family():
            seen |= set(t.verdicts(S, Q, n, rel, abs_).tolist())
            if name.startswith("cancellation") or name in ("non-finite", "zero n=2", "zero n=3", "subnormal n=3"):
                assert set(t.verdicts(S, Q, n, rel, abs_).tolist()) == {True, False}, name
        assert seen == {True, False}, family.__name__
    groups, sensitive = t.contraction_groups()
    total = sum(int(s.sum()) for s in sensitive)
    assert total >= 10_000, total
    fused_stops = sum(int((s & ~t.verdicts(S, Q, n, rel, abs_)).sum()) for (name, S, Q, n, rel, abs_), s in zip(groups, sensitive))
    assert 1000 < fused_stops < total - 1000, (fused_stops, total)  # the fused verdict errs in both directions
    assert all(s.mean() > 0.1 for s in sensitive), [float(s.mean()) for s in sensitive]
    # (a group's threshold sits a quarter of an ulp to one side of its two-rounding values: one verdict per group, both in the family)
    assert {bool(t.verdicts(S, Q, n, rel, abs_).all()) for name, S, Q, n, rel, abs_ in groups} == {True, False}
    assert all(len(set(t.verdicts(S, Q, n, rel, abs_).tolist())) == 1 for name, S, Q, n, rel, abs_ in groups)
