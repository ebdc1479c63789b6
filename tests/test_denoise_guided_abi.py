"""The surface-ID scene and the edge-guided denoiser without a GPU: rt_surface_id_tables against the Python statement of its rule on
every host scene (palette values, numbering order, only the named fields rewritten), every invalid argument of it and of
rt_denoise_guided_device (the field named, nothing written, no device touched), the sized initialiser and the workspace sizes, the
numpy restatement of the filter (guided_helpers) against exact rational arithmetic rounded once per operation and against the plain
and the albedo-guided restatements where the edge guide is constant, and the oracle's word that an ID scene's paths end at their
first hit."""
import ctypes as C
import math
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import albedo_helpers as ah
import denoise_helpers as dh
import guided_helpers as gh
import scene_cases
from adaptive_helpers import assert_bits

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_surface_id_tables", "rt_scene_create_surface_ids", "rt_denoise_guided_params_init_sized", "rt_denoise_guided_workspace_bytes",
           "rt_denoise_guided_device")
GUARD = 0x5A


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
    m = re.search(r"pub struct rt_denoise_guided_params\s*\{(.*?)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in rt.DenoiseGuidedParams._fields_]
    assert re.search(r"#define RT_SURFACE_ID_COLOURS 26\b", header) and rt.RT_SURFACE_ID_COLOURS == gh.COLOURS == 26
    for name in ("surface_id_tables", "surface_id_camera", "denoise_guided_params", "denoise_guided_workspace_bytes", "denoise_guided_device",
                 "denoise_guided"):
        assert callable(getattr(rt, name)), name


def test_rt_denoise_guided_params_has_gccs_layout(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(rt_denoise_guided_params));']
    for fname, _ in rt.DenoiseGuidedParams._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rt_denoise_guided_params, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(rt.DenoiseGuidedParams) == 48
    for fname, _ in rt.DenoiseGuidedParams._fields_:
        assert int(got[fname]) == getattr(rt.DenoiseGuidedParams, fname).offset, fname
    # the albedo params are a prefix: a caller may hand the same bytes to either filter
    assert [f for f, _ in rt.DenoiseGuidedParams._fields_][:6] == [f for f, _ in rt.DenoiseAlbedoParams._fields_]


# ---- the palette ----
def test_the_palette_is_26_exact_colours_without_black_at_least_half_apart():
    cols = [gh.palette(q) for q in range(1, 27)]
    assert len(set(cols)) == 26 and (0.0, 0.0, 0.0) not in cols and (1.0, 1.0, 1.0) in cols
    assert all(c in (0.0, 0.5, 1.0) for col in cols for c in col)
    assert cols[0] == (0.5, 0.0, 0.0) and cols[2] == (0.0, 0.5, 0.0) and cols[8] == (0.0, 0.0, 0.5) and cols[25] == (1.0, 1.0, 1.0)
    for i, a in enumerate(cols):
        for b in cols[i + 1:] + [(0.0, 0.0, 0.0)]:   # (and the background the layers above render with)
            assert max(abs(x - y) for x, y in zip(a, b)) >= 0.5


# ---- rt_surface_id_tables ----
HOST_SCENES = ["c2_random_balls_96x64_8spp_d50", "two_spheres_80x45_8spp", "earth_80x45_8spp", "two_perlin_spheres_80x45_8spp", "quads_64x64_8spp",
               "simple_light_80x45_16spp", "ragged_cornell_37x37_4spp", "cornell_smoke_64x64_16spp", "c4_final_scene_64x64_8spp_d40"]


def _buffers(rt, desc):
    sizes = [max(desc.n_spheres, 0) * C.sizeof(rt.Sphere), max(desc.n_quads, 0) * C.sizeof(rt.Quad), max(desc.n_media, 0) * C.sizeof(rt.ConstantMedium),
             26 * C.sizeof(rt.Material), 26 * C.sizeof(rt.Texture)]
    return sizes, [(C.c_uint8 * (n + 64))(*([GUARD] * (n + 64))) for n in sizes]


def _call_rule(rt, desc):
    """rt_surface_id_tables into guarded buffers: (rc, [spheres, quads, media, materials, textures] as bytes)"""
    sizes, bufs = _buffers(rt, desc)
    rc = rt.amd_lib().rt_surface_id_tables(C.byref(desc), *[C.addressof(b) for b in bufs])
    raw = [bytes(b) for b in bufs]
    for name, n, r in zip(("out_spheres", "out_quads", "out_media", "out_materials", "out_textures"), sizes, raw):
        assert r[n:] == bytes([GUARD]) * 64, f"bytes behind {name} were written"
    return rc, [r[:n] for n, r in zip(sizes, raw)]


def _tables(d):
    return (ah.table_bytes(d.spheres, d.n_spheres), ah.table_bytes(d.quads, d.n_quads), ah.table_bytes(d.media, d.n_media),
            ah.table_bytes(d.materials, d.n_materials), ah.table_bytes(d.textures, d.n_textures))


def _check_rule(rt, hs):
    d = hs.desc
    before = _tables(d)
    rc, got = _call_rule(rt, d)
    assert rc == 0, rt.amd_lib().rt_last_error()
    want = gh.id_rule(rt, d)
    for name, g, w in zip(("spheres", "quads", "media", "materials", "textures"), got, want):
        assert g == b"".join(bytes(x) for x in w), f"{name} differ from the rule"
    assert _tables(d) == before, "the input tables changed"
    # only the named field is rewritten: with it put back, every record is the original's
    spheres = (rt.Sphere * max(1, d.n_spheres)).from_buffer_copy(got[0] + bytes(C.sizeof(rt.Sphere)))
    quads = (rt.Quad * max(1, d.n_quads)).from_buffer_copy(got[1] + bytes(C.sizeof(rt.Quad)))
    media = (rt.ConstantMedium * max(1, d.n_media)).from_buffer_copy(got[2] + bytes(C.sizeof(rt.ConstantMedium)))
    k = 0
    for i in range(d.n_spheres):
        assert spheres[i].material == k % 26
        spheres[i].material = d.spheres[i].material
        k += 1
    for i in range(d.n_quads):
        assert quads[i].material == k % 26
        quads[i].material = d.quads[i].material
        k += 1
    for i in range(d.n_media):
        assert media[i].phase_material == k % 26
        media[i].phase_material = d.media[i].phase_material
        k += 1
    assert (bytes(spheres)[:len(before[0])], bytes(quads)[:len(before[1])], bytes(media)[:len(before[2])]) == before[:3]
    # the palette: material i is a light of texture i, texture i the solid of palette entry i + 1, every other field zeroed as the albedo rule zeroes it
    mats = (rt.Material * 26).from_buffer_copy(got[3])
    texs = (rt.Texture * 26).from_buffer_copy(got[4])
    for i in range(26):
        assert (mats[i].kind, mats[i].texture, mats[i].albedo.tuple(), mats[i].fuzz, mats[i].ir) == (rt.RT_MATERIAL_DIFFUSE_LIGHT, i, (0.0, 0.0, 0.0), 0.0, 0.0)
        t = texs[i]
        assert (t.kind, t.even, t.odd, t.image, t.perlin, t._pad, t.inv_scale, t.scale) == (rt.RT_TEXTURE_SOLID, -1, -1, -1, -1, 0, 0.0, 0.0)
        assert tuple(t.color.tuple()) == gh.palette(i + 1)
    # the Python binding is the same call
    assert [bytes(x) for x in rt.surface_id_tables(hs)] == got
    return k


@pytest.mark.parametrize("case", HOST_SCENES)
def test_rt_surface_id_tables_is_the_rule_on_every_host_scene(rt, case):
    hs = scene_cases.build(rt, case, width=16)
    n = _check_rule(rt, hs)
    assert n == hs.desc.n_spheres + hs.desc.n_quads + hs.desc.n_media > 0
    if case.startswith("cornell_smoke"):
        assert hs.desc.n_media == 2 and hs.desc.n_quads > 0, "media are numbered behind the quads"
    if case.startswith("c4_final_scene"):
        assert hs.desc.n_spheres > 26 and hs.desc.n_quads > 26 and hs.desc.n_media > 0, "all three tables, each longer than the palette"


def test_27_consecutive_surfaces_get_26_distinct_colours_and_the_first_again(rt):
    hs = scene_cases.build(rt, "c4_final_scene_64x64_8spp_d40", width=16)
    spheres, quads, media, mats, texs = rt.surface_id_tables(hs)
    d = hs.desc
    used = [s.material for s in spheres] + [q.material for q in quads] + [m.phase_material for m in media]
    assert len(used) >= 27 + d.n_spheres, "the run below crosses from the spheres into the quads"
    colour = lambda k: tuple(texs[mats[used[k]].texture].color.tuple())
    for first in (0, 5, d.n_spheres - 3, len(used) - 27):   # (a run inside the spheres, one across spheres / quads, one that ends in the media)
        run = [colour(first + j) for j in range(27)]
        assert len(set(run[:26])) == 26, first
        assert run[26] == run[0], first


def test_every_invalid_argument_of_rt_surface_id_tables_is_named_and_nothing_is_written(rt):
    lib = rt.amd_lib()
    hs = scene_cases.build(rt, "cornell_smoke_64x64_16spp", width=16)
    d = hs.desc

    def variant(**fields):
        v = rt.SceneDesc.from_buffer_copy(d)
        for k, val in fields.items():
            setattr(v, k, val)
        return v

    def null(field):
        v = rt.SceneDesc.from_buffer_copy(d)
        setattr(v, field, None)
        return v

    cases = [
        (dict(desc=None), "desc is null"), (dict(skip=0), "out_spheres is null"), (dict(skip=1), "out_quads is null"),
        (dict(skip=2), "out_media is null"), (dict(skip=3), "out_materials is null"), (dict(skip=4), "out_textures is null"),
        (dict(desc=variant(abi_version=1)), "abi_version"), (dict(desc=variant(abi_version=rt.RT_ABI_VERSION + 1)), "abi_version"),
        (dict(desc=variant(n_spheres=-1)), "n_spheres"), (dict(desc=variant(n_spheres=3, spheres=None)), "spheres"),
        (dict(desc=variant(n_quads=-5)), "n_quads"), (dict(desc=null("quads")), "quads"),
        (dict(desc=variant(n_media=-1)), "n_media"), (dict(desc=null("media")), "media"),
    ]
    for kw, field in cases:
        desc = kw.get("desc", d)
        sizes, bufs = _buffers(rt, d)
        ptrs = [C.addressof(b) for b in bufs]
        if "skip" in kw:
            ptrs[kw["skip"]] = None
        rc = lib.rt_surface_id_tables(C.byref(desc) if desc is not None else None, *ptrs)
        msg = lib.rt_last_error().decode()
        assert rc == -1, (field, rc, msg)
        assert field in msg and msg.startswith("rt_surface_id_tables: "), (field, msg)
        assert all(bytes(b) == bytes([GUARD]) * len(b) for b in bufs), f"{field}: something was written"
    # the checks come in the order the header states: of two faults the earlier one is named
    sizes, bufs = _buffers(rt, d)
    ptrs = [C.addressof(b) for b in bufs]
    assert lib.rt_surface_id_tables(C.byref(variant(abi_version=1, n_spheres=-1)), *ptrs) == -1 and "abi_version" in lib.rt_last_error().decode()
    assert lib.rt_surface_id_tables(C.byref(variant(n_spheres=-1, n_media=-1)), *ptrs) == -1 and "n_spheres" in lib.rt_last_error().decode()
    assert lib.rt_surface_id_tables(C.byref(variant(abi_version=1)), None, *ptrs[1:]) == -1 and "out_spheres" in lib.rt_last_error().decode()
    # rt_scene_create_surface_ids refuses the same descriptions before it looks for a device
    out = C.c_void_p()
    for desc, field in ((variant(abi_version=1), "abi_version"), (null("quads"), "quads"), (variant(n_media=-1), "n_media")):
        assert lib.rt_scene_create_surface_ids(C.byref(desc), 0, None, C.byref(out)) == -1
        assert field in lib.rt_last_error().decode() and not out.value
    assert lib.rt_scene_create_surface_ids(None, 0, None, C.byref(out)) == -1 and lib.rt_scene_create_surface_ids(C.byref(d), 0, None, None) == -1
    assert _call_rule(rt, d)[0] == 0


# ---- rt_denoise_guided_params, the workspace, rt_denoise_guided_device's refusals ----
def test_init_sized_writes_the_defaults_into_struct_size_bytes_only(rt):
    lib = rt.amd_lib()
    d = rt.denoise_guided_params()
    assert (d.struct_size, d.iterations, d.sigma, d.eps, d.sigma_edge) == (48, 4, 4.0, 1e-6, 0.5)
    assert gh.DEFAULTS == dict(iterations=d.iterations, sigma=d.sigma, eps=d.eps, sigma_albedo=d.sigma_albedo, albedo_floor=d.albedo_floor,
                               sigma_edge=d.sigma_edge)
    a = rt.denoise_albedo_params()
    assert bytes(d)[4:40] == bytes(a)[4:40], "the shared fields have the albedo filter's defaults"
    full = bytes(d)
    for size in (8, 16, 24, 32, 40, 48):
        buf = (C.c_uint8 * 64)(*([0xA5] * 64))
        assert lib.rt_denoise_guided_params_init_sized(buf, size) == 0
        raw = bytes(buf)
        assert raw[size:] == b"\xa5" * (64 - size), size
        assert raw[4:size] == full[4:size] and int.from_bytes(raw[:4], "little") == size, size
    for size in (0, 4, 12, 44, 49, 56):
        buf = (C.c_uint8 * 64)(*([0xA5] * 64))
        assert lib.rt_denoise_guided_params_init_sized(buf, size) == -1, size
        assert "struct_size" in lib.rt_last_error().decode()
        assert bytes(buf) == b"\xa5" * 64
    assert lib.rt_denoise_guided_params_init_sized(None, 48) == -1
    with pytest.raises(TypeError):
        rt.denoise_guided_params(radius=3)


def test_the_workspace_holds_three_or_four_regions_and_refuses_2_to_the_27_pixels(rt):
    lib = rt.amd_lib()
    for w, h in [(1, 1), (5, 3), (17, 9), (70, 37), (130, 66), (1200, 800), ((1 << 14) - 1, 1 << 13)]:
        assert lib.rt_denoise_guided_workspace_bytes(w, h, 0) == 3 * 4 * 8 * w * h == lib.rt_denoise_albedo_workspace_bytes(w, h)
        assert lib.rt_denoise_guided_workspace_bytes(w, h, 1) == 4 * 4 * 8 * w * h == lib.rt_denoise_guided_workspace_bytes(w, h, 7)
        assert rt.denoise_guided_workspace_bytes(w, h, True) == 4 * 4 * 8 * w * h and rt.denoise_guided_workspace_bytes(w, h, False) == 3 * 4 * 8 * w * h
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 14, 1 << 13), (1 << 27, 1), (1 << 20, 1 << 20)):
        for with_albedo in (0, 1):
            assert lib.rt_denoise_guided_workspace_bytes(w, h, with_albedo) == -1
            with pytest.raises(rt.RtError):
                rt.denoise_guided_workspace_bytes(w, h, with_albedo)


def _denoise(rt, *, w=6, h=4, s=True, q=True, a=True, e=True, spp=8, aspp=8, espp=8, spp_map=False, params=None, out=True, rgba=True, ws=True,
             alias=None, misalign=False, ws_misalign=False):
    """One call of rt_denoise_guided_device on HOST buffers: only argument checks can answer (the first thing past them asks the HIP
    runtime which device owns d_mean_out, and host memory has none).  Returns (rc, message, the output buffer's bytes)."""
    lib = rt.amd_lib()
    n = w * h if w > 0 and h > 0 and w * h < (1 << 20) else 1
    S, Q, A, E = ((C.c_double * (3 * n))() for _ in range(4))
    M = (C.c_uint8 * (24 * n))(*([GUARD] * (24 * n)))
    N = (C.c_int32 * n)()
    B = (C.c_uint8 * (4 * n + 4))()
    W = (C.c_uint8 * (128 * n + 32))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    out_ptr = {None: C.addressof(M), "sum": C.addressof(S) + 8 * (3 * n - 1), "sum_sq": C.addressof(Q), "albedo": C.addressof(A) + 8 * (3 * n - 1),
               "edge": C.addressof(E) + 8 * (3 * n - 1), "edge0": C.addressof(E)}[alias]
    rc = lib.rt_denoise_guided_device(w, h, C.addressof(S) if s else None, C.addressof(Q) if q else None, spp, C.addressof(N) if spp_map else None,
                                      C.addressof(A) if a else None, aspp, C.addressof(E) if e else None, espp,
                                      C.byref(params) if params is not None else None, out_ptr if out else None,
                                      (C.addressof(B) + (1 if misalign else 0)) if rgba else None, ws_ptr if ws else None, None)
    return rc, lib.rt_last_error().decode(), bytes(M)


def test_every_invalid_denoise_guided_argument_is_named_without_a_device(rt):
    P, dp = rt.DenoiseGuidedParams, rt.denoise_guided_params
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(s=False), "d_sum is null"), (dict(q=False), "d_sum_sq is null"), (dict(e=False), "d_edge_sum is null"),
        (dict(e=False, a=False), "d_edge_sum is null"),
        (dict(out=False), "d_mean_out is null"), (dict(ws=False), "d_workspace is null"),
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(spp=1), "spp"), (dict(spp=0), "spp"), (dict(spp=-4), "spp"),
        (dict(aspp=0), "albedo_spp"), (dict(aspp=-1), "albedo_spp"),
        (dict(espp=0), "edge_spp"), (dict(espp=-1), "edge_spp"), (dict(espp=0, a=False), "edge_spp"),
        (dict(params=P(struct_size=12, iterations=4, sigma=4.0, eps=1e-6)), "rt_denoise_guided_params.struct_size"),
        (dict(params=P(struct_size=56, iterations=4, sigma=4.0, eps=1e-6, sigma_albedo=1.0, albedo_floor=0.1, sigma_edge=0.5)), "struct_size"),
        (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=dp(iterations=0)), "iterations"), (dict(params=dp(iterations=7)), "iterations"),
        (dict(params=dp(sigma=0.0)), "sigma"), (dict(params=dp(sigma=nan)), "sigma"), (dict(params=dp(sigma=inf)), "sigma"),
        (dict(params=dp(eps=0.0)), "eps"), (dict(params=dp(eps=nan)), "eps"),
        (dict(params=dp(sigma_albedo=0.0)), "sigma_albedo"), (dict(params=dp(sigma_albedo=nan)), "sigma_albedo"),
        (dict(params=dp(albedo_floor=0.0)), "albedo_floor"), (dict(params=dp(albedo_floor=inf)), "albedo_floor"),
        (dict(params=dp(sigma_edge=0.0)), "sigma_edge"), (dict(params=dp(sigma_edge=-0.5)), "sigma_edge"),
        (dict(params=dp(sigma_edge=nan)), "sigma_edge"), (dict(params=dp(sigma_edge=inf)), "sigma_edge"),
        (dict(params=dp(sigma_edge=0.0), a=False), "sigma_edge"),
        (dict(alias="sum"), "d_mean_out"), (dict(alias="sum_sq"), "d_mean_out"), (dict(alias="albedo"), "d_albedo_sum"),
        (dict(alias="edge"), "d_edge_sum"), (dict(alias="edge0"), "d_edge_sum"), (dict(alias="edge", a=False), "d_edge_sum"),
        (dict(misalign=True), "d_rgba8"), (dict(ws_misalign=True), "d_workspace"),
    ]
    for kw, field in cases:
        rc, msg, out = _denoise(rt, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith("rt_denoise_guided_device: "), (kw, msg)
        assert out == bytes([GUARD]) * len(out), (kw, "the output buffer was written")
    # the documented order: of two faults the earlier one is named
    for kw, field in ((dict(e=False, out=False), "d_edge_sum"), (dict(aspp=0, espp=0), "albedo_spp"), (dict(espp=0, params=dp(iterations=0)), "edge_spp"),
                      (dict(params=dp(albedo_floor=0.0, sigma_edge=0.0)), "albedo_floor"), (dict(params=dp(sigma_edge=0.0), alias="sum"), "sigma_edge"),
                      (dict(alias="edge", misalign=True), "d_edge_sum")):
        rc, msg, _ = _denoise(rt, **kw)
        assert rc == -1 and field in msg, (kw, msg)
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer.
    # Without an albedo frame its count and its two parameters are not read.
    for kw in (dict(), dict(rgba=False), dict(a=False), dict(spp=1, spp_map=True), dict(spp=2, aspp=1, espp=1), dict(a=False, aspp=0),
               dict(a=False, aspp=-7, params=dp(sigma_albedo=0.0, albedo_floor=nan)), dict(params=dp(iterations=6)),
               dict(params=dp(iterations=1, sigma=0.5, eps=1e-12, sigma_albedo=1e-9, albedo_floor=1e-300, sigma_edge=1e-9)),
               dict(params=P(struct_size=8, iterations=2)), dict(params=P(struct_size=40, iterations=2, sigma=1.0, eps=1e-3, sigma_albedo=0.7, albedo_floor=0.1))):
        rc, msg, out = _denoise(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)
        assert out == bytes([GUARD]) * len(out)
    # a shorter struct's missing fields are the defaults, not the bytes behind it
    rc, msg, _ = _denoise(rt, params=P(struct_size=40, iterations=2, sigma=1.0, eps=1e-3, sigma_albedo=0.7, albedo_floor=0.1, sigma_edge=nan))
    assert "not a device pointer" in msg, msg


# ---- the numpy restatement ----
def _r(x):
    return float(x)  # Fraction -> the nearest double, ties to even: one correctly rounded operation


def _F(x):
    return Fraction(x)


def _exact_row(S, Q, n, E, n_e, A, n_a, sigma, eps, sigma_albedo, floor, sigma_edge):
    """A W x 1 frame (W <= 3), one iteration at stride 1, in exact rational arithmetic rounded after every operation (a square root:
    the correctly rounded one of the rounded argument, checked by squaring its neighbours).  A None: no albedo frame.  Returns
    (out (W, 3) as floats, the edge stops eg seen, the tap factors that were (e * ea) * eg products)."""
    W = len(S)
    mx = lambda a, b: b if b > a else a
    m = [[_r(_F(s) / n) for s in S[p]] for p in range(W)]
    g = [[_r(_F(x) / n_e) for x in E[p]] for p in range(W)]
    v = [[_r(_F(_r(_F(Q[p][c]) - _F(_r(_F(S[p][c]) * _F(m[p][c]))))) / (n - 1)) for c in range(3)] for p in range(W)]
    if A is None:
        I, u, d, a = m, v, None, None
    else:
        a = [[_r(_F(x) / n_a) for x in A[p]] for p in range(W)]
        d = [[mx(x, floor) for x in a[p]] for p in range(W)]
        I = [[_r(_F(m[p][c]) / _F(d[p][c])) for c in range(3)] for p in range(W)]
        u = [[_r(_F(v[p][c]) / _F(_r(_F(d[p][c]) * _F(d[p][c])))) for c in range(3)] for p in range(W)]
    V = [_r(_F(mx(mx(mx(u[p][0], u[p][1]), u[p][2]), 0.0)) / n) for p in range(W)]
    L = [_r(_F(_r(_F(_r(_F(I[p][0]) + _F(I[p][1]))) + _F(I[p][2]))) / 3) for p in range(W)]

    def stop(x, p, q, width):
        dd = mx(mx(_r(abs(_F(x[p][0]) - _F(x[q][0]))), _r(abs(_F(x[p][1]) - _F(x[q][1])))), _r(abs(_F(x[p][2]) - _F(x[q][2]))))
        z = _r(_F(dd) / _F(width))
        t = _r(1 - _F(_r(_F(z) * _F(z))))
        return _r(_F(t) * _F(t)) if t > 0.0 else 0.0

    out, egs, products = [], [], []
    for p in range(W):
        gs, ws = 0.0, 0.0
        for dx in (-1, 0, 1):   # the prefilter: row dy = 0 only (the frame is one row), g[1] = 1/2 times g[dx]
            q = p + dx
            if not 0 <= q < W:
                continue
            k = 0.5 * (0.25, 0.5, 0.25)[dx + 1]
            gs = _r(_F(gs) + _F(_r(_F(k) * _F(V[q]))))
            ws = _r(_F(ws) + _F(k))
        G = _r(_F(gs) / _F(ws))
        sd = math.sqrt(G)
        for cand in (np.nextafter(sd, 0.0), np.nextafter(sd, np.inf)):  # math.sqrt is IEEE: its neighbours are further from the root
            assert abs(_F(float(cand)) ** 2 - _F(G)) >= abs(_F(sd) ** 2 - _F(G))
        den = _r(_F(_r(_F(sigma) * _F(sd))) + _F(eps))
        sw, sv, sc = 0.0, 0.0, [0.0, 0.0, 0.0]
        for dx in (-2, -1, 0, 1, 2):
            q = p + dx
            if not 0 <= q < W:
                continue
            x = _r(_F(_r(abs(_F(L[p]) - _F(L[q])))) / _F(den))
            t = _r(1 - _F(_r(_F(x) * _F(x))))
            e = _r(_F(t) * _F(t)) if t > 0.0 else 0.0
            eg = stop(g, p, q, sigma_edge)
            egs.append(eg)
            if A is None:
                f = _r(_F(e) * _F(eg))
            else:
                ea = stop(a, p, q, sigma_albedo)
                f = _r(_F(_r(_F(e) * _F(ea))) * _F(eg))
                products.append((e, ea, eg))
            hh = _r(_F(dh.H5[2]) * _F(dh.H5[dx + 2]))
            wq = _r(_F(hh) * _F(f))
            sw = _r(_F(sw) + _F(wq))
            for c in range(3):
                sc[c] = _r(_F(sc[c]) + _F(_r(_F(wq) * _F(I[q][c]))))
            sv = _r(_F(sv) + _F(_r(_F(_r(_F(wq) * _F(wq))) * _F(V[q]))))
        C1 = [_r(_F(sc[c]) / _F(sw)) for c in range(3)]
        out.append(C1 if A is None else [_r(_F(C1[c]) * _F(d[p][c])) for c in range(3)])
    return out, egs, products


ROW_S = [[0.7, 2.3, 1.1], [0.9, 2.0, 1.3], [0.8, 2.2, 1.0]]
ROW_Q = [[0.41, 1.9, 0.52], [0.45, 1.7, 0.66], [0.43, 1.8, 0.5]]
ROW_A = [[1.3, 2.9, 0.8], [1.9, 2.2, 0.3], [1.5, 2.6, 0.7]]
# edge sums of n_e = 4 samples: pixel 0 wholly on one surface (0.5, 0, 1), pixel 1 three samples on it and one on (1, 0, 1) — its mean
# is 0.125 from pixel 0's, so 0 < eg < 1 at sigma_edge 0.5 — and pixel 2 wholly on (1, 0.5, 1): 0.5 from pixel 0's, eg = 0
ROW_E = [[2.0, 0.0, 4.0], [2.5, 0.0, 4.0], [4.0, 2.0, 4.0]]


@pytest.mark.parametrize("with_albedo", [False, True])
@pytest.mark.parametrize("width, sigma_edge", [(2, 0.5), (3, 0.5), (3, 0.3), (3, 2.0)])
def test_the_numpy_statement_is_the_definition_rounded_once_per_operation(width, sigma_edge, with_albedo):
    """Two or three pixels in a row whose edge guides differ by 0.125 and by 0.375 / 0.5: the stop reaches eg = 1 (the centre),
    0 < eg < 1 and, at sigma_edge <= 0.5, eg = 0; with an albedo frame every tap's factor is the product (e * ea) * eg."""
    S, Q, E = ROW_S[:width], ROW_Q[:width], ROW_E[:width]
    A = ROW_A[:width] if with_albedo else None
    n, n_e, n_a = 3, 4, 4
    want, egs, products = _exact_row(S, Q, n, E, n_e, A, n_a, 4.0, 1e-6, 0.5, 1e-3, sigma_edge)
    got = gh.denoise_guided(np.array([S]), np.array([Q]), n, np.array([E]), n_e, None if A is None else np.array([A]), n_a, iterations=1,
                            sigma_edge=sigma_edge)
    assert [[float(x).hex() for x in px] for px in got[0]] == [[x.hex() for x in px] for px in want]
    assert 1.0 in egs and any(0.0 < x < 1.0 for x in egs)
    if width == 3 and sigma_edge <= 0.5:
        assert 0.0 in egs
    if width == 3 and sigma_edge == 2.0:
        assert 0.0 not in egs
    if with_albedo:
        assert any(0.0 < e < 1.0 and 0.0 < ea < 1.0 and 0.0 < eg < 1.0 for e, ea, eg in products), "no tap had all three factors inside (0, 1)"
    if width == 3 and sigma_edge == 0.3:  # pixel 2 is 0.375 or more from both others: no tap of it, and it is no tap
        alone = gh.denoise_guided(np.array([S[2:]]), np.array([Q[2:]]), n, np.array([E[2:]]), n_e, None if A is None else np.array([A[2:]]), n_a,
                                  iterations=1, sigma_edge=sigma_edge)
        # (its variance prefilter still reads pixel 1's V, so only the colour of a pixel filtered alone is comparable where V plays no part:
        #  a single tap of weight w gives (w * C) / w)
        wq = 9.0 / 64.0
        C0 = gh.prepare(np.array([S]), np.array([Q]), n, np.array([E]), n_e, None if A is None else np.array([A]), n_a)[0]
        d = gh.prepare(np.array([S]), np.array([Q]), n, np.array([E]), n_e, None if A is None else np.array([A]), n_a)[5]
        one_tap = (wq * C0[0, 2]) / wq
        assert_bits(got[0, 2], one_tap if d is None else one_tap * d[0, 2], "eg = 0 on both sides: the centre is the only tap")
        assert_bits(alone[0, 0], got[0, 2], "and that is the pixel filtered alone")


def test_pixels_that_are_not_valid_keep_their_mean_and_are_no_taps():
    S, Q, spp, spp_map = dh.synthetic(17, 9, 3)
    A, n_a = ah.synthetic_albedo(17, 9, 4)
    E, n_e = gh.synthetic_edges(17, 9, 5)
    for alb in (None, A):
        out = gh.denoise_guided(S, Q, spp_map, E, n_e, alb, n_a)
        valid = gh.prepare(S, Q, spp_map, E, n_e, alb, n_a)[2]
        assert valid.any() and not valid.all() and (~np.isfinite(E)).any() and (spp_map < 2).any()
        only_e = ~np.isfinite(E).all(axis=2) & np.isfinite(S).all(axis=2) & np.isfinite(Q).all(axis=2) & (spp_map >= 2)
        assert only_e.any() and not valid[only_e].any(), "a non-finite E alone makes a pixel not valid"
        with np.errstate(all="ignore"):
            m = S / spp_map.astype(np.float64)[:, :, None]
        assert_bits(out[~valid], m[~valid], "a pixel that is not valid is written unchanged")
        assert np.isfinite(out[valid]).all(), "a valid pixel took a tap that is not valid"


@pytest.mark.parametrize("w, h, k", [(1, 1, 1), (5, 3, 2), (17, 9, 4), (70, 37, 4), (40, 21, 6)])
def test_a_constant_edge_guide_is_the_plain_and_the_albedo_guided_filter_bit_for_bit(w, h, k):
    S, Q, spp, spp_map = dh.synthetic(w, h, 1000 * w + h)
    A, n_a = ah.synthetic_albedo(w, h, 77 * w + h)
    for n_e, colour in ((1, (0.0, 0.0, 0.0)), (3, (0.5, 1.0, 0.0)), (16, (1.0, 1.0, 1.0))):
        E = np.broadcast_to(np.array(colour) * n_e, (h, w, 3))
        for n in (spp, spp_map):
            assert_bits(gh.denoise_guided(S, Q, n, E, n_e, iterations=k), dh.denoise(S, Q, n, iterations=k), f"{w}x{h}, K = {k}, n_e = {n_e}: plain")
            assert_bits(gh.denoise_guided(S, Q, n, E, n_e, A, n_a, iterations=k), ah.denoise_albedo(S, Q, n, A, n_a, iterations=k),
                        f"{w}x{h}, K = {k}, n_e = {n_e}: albedo-guided")
    E = np.full((h, w, 3), 0.3)
    assert_bits(gh.denoise_guided(S, Q, spp, E, 7, iterations=k, sigma=1.5, eps=1e-3, sigma_edge=1e-9), dh.denoise(S, Q, spp, iterations=k, sigma=1.5, eps=1e-3),
                "other parameters, a guide that is no palette colour")
    assert_bits(gh.denoise_guided(S, Q, spp, E, 7, A, n_a, iterations=k, sigma_albedo=0.7, albedo_floor=0.3, sigma_edge=1e-9),
                ah.denoise_albedo(S, Q, spp, A, n_a, iterations=k, sigma_albedo=0.7, albedo_floor=0.3), "other parameters, with an albedo frame")
    if w * h >= 15:
        Es, n_es = gh.synthetic_edges(w, h, 5)
        assert not np.array_equal(gh.denoise_guided(S, Q, spp, Es, n_es, iterations=k), dh.denoise(S, Q, spp, iterations=k), equal_nan=True)


def test_no_tap_crosses_a_step_of_the_guide_that_is_sigma_edge_or_more():
    """A guide of two flat halves one apart (the albedo frame of two materials, say, fed as the edge guide): when the right half's
    moments change, no pixel of the left half moves by a bit, but for the column at the step, whose 3 x 3 prefilter of the variance
    (no tap: it takes no stop) reaches across."""
    w, h = 17, 9
    S, Q, spp, _ = dh.synthetic(w, h, 3)
    rng = np.random.default_rng(8)
    A = np.where(np.arange(w)[None, :, None] < w // 2, 1.0, 2.0) * np.ones((h, w, 3)) * 4.0
    edges = gh.denoise_guided(S, Q, spp, A, 4, iterations=1)
    plain = dh.denoise(S, Q, spp, iterations=1)
    assert not np.array_equal(edges, plain, equal_nan=True)
    S2 = S.copy()
    S2[:, w // 2:] = S[:, w // 2:] * 1.5 + rng.random((h, w - w // 2, 3))
    edges2 = gh.denoise_guided(S2, Q, spp, A, 4, iterations=1)
    valid = gh.prepare(S, Q, spp, A, 4)[2] & gh.prepare(S2, Q, spp, A, 4)[2]
    left = np.zeros((h, w), dtype=bool)
    left[:, :w // 2 - 1] = True   # (the column at the edge reads its neighbour's V in the variance prefilter)
    assert_bits(edges2[left & valid], edges[left & valid], "a step of 1.0 in the guide at sigma_edge 0.5: no tap crosses it")


# ---- the oracle's word on what an ID scene's render is ----
def test_the_oracles_paths_through_an_id_scene_end_at_the_first_hit(rt, oracle):
    for case, over in (("ragged_cornell_37x37_4spp", {}), ("cornell_smoke_64x64_16spp", dict(width=24, spp=4))):
        hs = scene_cases.build(rt, case, **over)
        assert hs.camera.max_depth == 8
        ids = gh.SurfaceIdScene(rt, hs)
        assert tuple(ids.camera.background.tuple()) == (0.0, 0.0, 0.0) and bytes(hs.desc) != bytes(ids.desc)
        one = oracle.render(ids, rt.render_params(seed=9, sample_end=4, max_depth=1))
        eight = oracle.render(ids, rt.render_params(seed=9, sample_end=4, max_depth=8))
        assert_bits(one, eight, f"{case}: max_depth 1 against max_depth 8")
        # at one sample every pixel is exactly a palette colour or the background
        colours = {tuple(c) for c in oracle.render(ids, rt.render_params(seed=9, sample_end=1)).reshape(-1, 3).tolist()}
        allowed = {gh.palette(q) for q in range(1, 27)} | {(0.0, 0.0, 0.0)}
        assert colours <= allowed and len(colours) >= 4, colours
        if case.startswith("cornell_smoke"):
            d = hs.desc
            media = {gh.palette((d.n_spheres + d.n_quads + i) % 26 + 1) for i in range(d.n_media)}
            assert media <= colours, "no path ended inside a medium"
        # and the beauty render of the original does depend on the depth: the identity above is the ID scene's
        assert not np.array_equal(oracle.render(hs, rt.render_params(seed=9, sample_end=4, max_depth=1)),
                                  oracle.render(hs, rt.render_params(seed=9, sample_end=4, max_depth=8)))
