"""The albedo scene and the albedo-guided denoiser without a GPU: rt_albedo_materials against the Python statement of its rule on
every host scene, every invalid argument of it and of rt_denoise_albedo_device (the field named, no device touched), the sized
initialiser and the workspace size, the numpy restatement of the filter (albedo_helpers) against exact rational arithmetic rounded
once per operation and against the plain filter's where the albedo is 1, and the oracle's word that an albedo scene's paths end at
their first hit."""
import ctypes as C
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import albedo_helpers as ah
import custom_scenes
import denoise_helpers as dh
import scene_cases
from adaptive_helpers import assert_bits

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_albedo_materials", "rt_scene_create_albedo", "rt_denoise_albedo_params_init_sized", "rt_denoise_albedo_workspace_bytes",
           "rt_denoise_albedo_device")
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
    m = re.search(r"pub struct rt_denoise_albedo_params\s*\{(.*?)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in rt.DenoiseAlbedoParams._fields_]
    for name in ("albedo_materials", "albedo_camera", "denoise_albedo_params", "denoise_albedo_workspace_bytes", "denoise_albedo_device", "denoise_albedo"):
        assert callable(getattr(rt, name)), name


def test_rt_denoise_albedo_params_has_gccs_layout(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(rt_denoise_albedo_params));']
    for fname, _ in rt.DenoiseAlbedoParams._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rt_denoise_albedo_params, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(rt.DenoiseAlbedoParams) == 40
    for fname, _ in rt.DenoiseAlbedoParams._fields_:
        assert int(got[fname]) == getattr(rt.DenoiseAlbedoParams, fname).offset, fname


# ---- rt_albedo_materials ----
HOST_SCENES = ["c2_random_balls_96x64_8spp_d50", "two_spheres_80x45_8spp", "earth_80x45_8spp", "two_perlin_spheres_80x45_8spp", "quads_64x64_8spp",
               "simple_light_80x45_16spp", "ragged_cornell_37x37_4spp", "cornell_smoke_64x64_16spp", "c4_final_scene_64x64_8spp_d40"]


def _call_rule(rt, desc):
    """rt_albedo_materials into guarded buffers: (rc, materials bytes, textures bytes, n_textures)"""
    lib = rt.amd_lib()
    msz, tsz = C.sizeof(rt.Material), C.sizeof(rt.Texture)
    nm, room = max(desc.n_materials, 0), max(desc.n_textures, 0) + max(desc.n_materials, 0)
    M = (C.c_uint8 * (nm * msz + 64))(*([GUARD] * (nm * msz + 64)))
    T = (C.c_uint8 * (room * tsz + 64))(*([GUARD] * (room * tsz + 64)))
    n = C.c_int32(-7)
    rc = lib.rt_albedo_materials(C.byref(desc), C.addressof(M), C.addressof(T), C.byref(n))
    m, t = bytes(M), bytes(T)
    assert m[nm * msz:] == bytes([GUARD]) * 64, "bytes behind out_materials were written"
    assert t[room * tsz:] == bytes([GUARD]) * 64, "bytes behind out_textures were written"
    return rc, m[:nm * msz], t[:room * tsz], n.value


def _check_rule(rt, hs):
    d = hs.desc
    before = (ah.table_bytes(d.materials, d.n_materials), ah.table_bytes(d.textures, d.n_textures))
    rc, m, t, n = _call_rule(rt, d)
    assert rc == 0, rt.amd_lib().rt_last_error()
    want_m, want_t = ah.albedo_rule(rt, d)
    kinds = [d.materials[k].kind for k in range(d.n_materials)]
    appended = sum(k in (rt.RT_MATERIAL_METAL, rt.RT_MATERIAL_DIELECTRIC) for k in kinds)
    assert n == d.n_textures + appended == len(want_t)
    assert m == b"".join(bytes(x) for x in want_m), "materials differ from the rule"
    tsz = C.sizeof(rt.Texture)
    assert t[:n * tsz] == b"".join(bytes(x) for x in want_t), "textures differ from the rule"
    assert t[n * tsz:] == bytes([GUARD]) * (len(t) - n * tsz), "textures beyond out_n_textures were written"
    out = (rt.Material * max(1, d.n_materials)).from_buffer_copy(m + bytes(C.sizeof(rt.Material)))
    assert all(out[k].kind == rt.RT_MATERIAL_DIFFUSE_LIGHT and 0 <= out[k].texture < n for k in range(d.n_materials))
    assert (ah.table_bytes(d.materials, d.n_materials), ah.table_bytes(d.textures, d.n_textures)) == before, "the input tables changed"
    # the Python binding is the same call
    pm, pt = rt.albedo_materials(hs)
    assert bytes(pm) == m and bytes(pt) == t[:n * tsz]
    return kinds, appended


@pytest.mark.parametrize("case", HOST_SCENES)
def test_rt_albedo_materials_is_the_rule_on_every_host_scene(rt, case):
    hs = scene_cases.build(rt, case, width=16)
    assert hs.desc.n_materials > 0
    kinds, appended = _check_rule(rt, hs)
    if case.startswith(("c2_random_balls", "c4_final_scene")):
        assert appended > 0 and rt.RT_MATERIAL_METAL in kinds and rt.RT_MATERIAL_DIELECTRIC in kinds
    if case.startswith(("simple_light", "ragged_cornell")):
        assert rt.RT_MATERIAL_DIFFUSE_LIGHT in kinds, "a light that is copied"
    if case.startswith("cornell_smoke"):
        assert rt.RT_MATERIAL_ISOTROPIC in kinds


def test_rt_albedo_materials_is_the_rule_on_65535_materials(rt):
    cam = scene_cases.build(rt, "ragged_cornell_37x37_4spp")
    hs = custom_scenes.many_materials_scene(cam, 65533)
    kinds, appended = _check_rule(rt, hs)
    assert len(kinds) == 65535 and appended == 2


def test_every_invalid_argument_of_rt_albedo_materials_is_named_without_a_device(rt):
    lib = rt.amd_lib()
    hs = scene_cases.build(rt, "c2_random_balls_96x64_8spp_d50", width=16)
    d = hs.desc
    M = (rt.Material * d.n_materials)()
    T = (rt.Texture * (d.n_textures + d.n_materials))()
    n = C.c_int32(-7)

    def call(desc=d, m=True, t=True, nn=True):
        rc = lib.rt_albedo_materials(C.byref(desc) if desc is not None else None, C.addressof(M) if m else None, C.addressof(T) if t else None,
                                     C.byref(n) if nn else None)
        return rc, lib.rt_last_error().decode()

    def variant(**fields):
        v = rt.SceneDesc.from_buffer_copy(d)
        mats = (rt.Material * d.n_materials).from_buffer_copy(C.string_at(C.addressof(d.materials.contents), d.n_materials * C.sizeof(rt.Material)))
        v.materials = mats
        v._keep = mats
        for k, val in fields.items():
            if k.startswith("mat_"):
                setattr(mats[3], k[4:], val)
            else:
                setattr(v, k, val)
        return v

    lambertian = next(k for k in range(d.n_materials) if d.materials[k].kind == rt.RT_MATERIAL_LAMBERTIAN)
    bad_tex = variant()
    bad_tex._keep[lambertian].texture = d.n_textures
    neg_tex = variant()
    neg_tex._keep[lambertian].texture = -1
    null_mats = rt.SceneDesc.from_buffer_copy(d)
    null_mats.materials = None
    cases = [
        (dict(desc=None), "desc is null"), (dict(m=False), "out_materials is null"), (dict(t=False), "out_textures is null"),
        (dict(nn=False), "out_n_textures is null"),
        (dict(desc=variant(abi_version=1)), "abi_version"), (dict(desc=variant(abi_version=rt.RT_ABI_VERSION + 1)), "abi_version"),
        (dict(desc=variant(mat_kind=0)), "materials[3].kind"), (dict(desc=variant(mat_kind=6)), "materials[3].kind"),
        (dict(desc=variant(mat_kind=-2)), "materials[3].kind"),
        (dict(desc=bad_tex), f"materials[{lambertian}].texture"), (dict(desc=neg_tex), f"materials[{lambertian}].texture"),
        (dict(desc=null_mats), "materials"), (dict(desc=variant(n_materials=-1)), "n_materials"),
    ]
    for kw, field in cases:
        rc, msg = call(**kw)
        assert rc == -1, (field, rc, msg)
        assert field in msg and msg.startswith("rt_albedo_materials: "), (field, msg)
        assert n.value == -7 and bytes(M) == bytes(C.sizeof(M)) and bytes(T) == bytes(C.sizeof(T)), f"{field}: something was written"
    # rt_scene_create_albedo refuses the same descriptions before it looks for a device
    out = C.c_void_p()
    for desc, field in ((variant(abi_version=1), "abi_version"), (variant(mat_kind=9), "materials[3].kind"), (bad_tex, "texture")):
        assert lib.rt_scene_create_albedo(C.byref(desc), 0, None, C.byref(out)) == -1
        assert field in lib.rt_last_error().decode() and not out.value
    assert lib.rt_scene_create_albedo(None, 0, None, C.byref(out)) == -1 and lib.rt_scene_create_albedo(C.byref(d), 0, None, None) == -1
    assert call()[0] == 0


# ---- rt_denoise_albedo_params, the workspace, rt_denoise_albedo_device's refusals ----
def test_init_sized_writes_the_defaults_into_struct_size_bytes_only(rt):
    lib = rt.amd_lib()
    d = rt.denoise_albedo_params()
    assert (d.struct_size, d.iterations, d.sigma, d.eps) == (40, 4, 4.0, 1e-6)
    assert ah.DEFAULTS == dict(iterations=d.iterations, sigma=d.sigma, eps=d.eps, sigma_albedo=d.sigma_albedo, albedo_floor=d.albedo_floor)
    assert 0.0 < d.albedo_floor <= 1.0 and d.sigma_albedo > 0.0
    full = bytes(d)
    for size in (8, 16, 24, 32, 40):
        buf = (C.c_uint8 * 56)(*([0xA5] * 56))
        assert lib.rt_denoise_albedo_params_init_sized(buf, size) == 0
        raw = bytes(buf)
        assert raw[size:] == b"\xa5" * (56 - size), size
        assert raw[4:size] == full[4:size] and int.from_bytes(raw[:4], "little") == size, size
    for size in (0, 4, 12, 36, 41, 48):
        buf = (C.c_uint8 * 56)(*([0xA5] * 56))
        assert lib.rt_denoise_albedo_params_init_sized(buf, size) == -1, size
        assert "struct_size" in lib.rt_last_error().decode()
        assert bytes(buf) == b"\xa5" * 56
    assert lib.rt_denoise_albedo_params_init_sized(None, 40) == -1
    with pytest.raises(TypeError):
        rt.denoise_albedo_params(radius=3)


def test_the_workspace_holds_three_regions_and_refuses_2_to_the_27_pixels(rt):
    lib = rt.amd_lib()
    for w, h in [(1, 1), (5, 3), (17, 9), (70, 37), (130, 66), (1200, 800), ((1 << 14) - 1, 1 << 13)]:
        assert lib.rt_denoise_albedo_workspace_bytes(w, h) == 3 * 4 * 8 * w * h
        assert lib.rt_denoise_albedo_workspace_bytes(w, h) == lib.rt_denoise_workspace_bytes(w, h) // 2 * 3
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 14, 1 << 13), (1 << 27, 1), (1 << 20, 1 << 20)):
        assert lib.rt_denoise_albedo_workspace_bytes(w, h) == -1
        with pytest.raises(rt.RtError):
            rt.denoise_albedo_workspace_bytes(w, h)


def _denoise(rt, *, w=6, h=4, s=True, q=True, a=True, spp=8, aspp=8, spp_map=False, params=None, out=True, rgba=True, ws=True, alias=None,
             misalign=False, ws_misalign=False):
    """One call of rt_denoise_albedo_device on HOST buffers: only argument checks can answer (the first thing past them asks the HIP
    runtime which device owns d_mean_out, and host memory has none)."""
    lib = rt.amd_lib()
    n = w * h if w > 0 and h > 0 and w * h < (1 << 20) else 1
    S, Q, A, M = ((C.c_double * (3 * n))() for _ in range(4))
    N = (C.c_int32 * n)()
    B = (C.c_uint8 * (4 * n + 4))()
    W = (C.c_uint8 * (96 * n + 32))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    out_ptr = {None: C.addressof(M), "sum": C.addressof(S) + 8 * (3 * n - 1), "sum_sq": C.addressof(Q), "albedo": C.addressof(A) + 8 * (3 * n - 1),
               "albedo0": C.addressof(A)}[alias]
    rc = lib.rt_denoise_albedo_device(w, h, C.addressof(S) if s else None, C.addressof(Q) if q else None, spp, C.addressof(N) if spp_map else None,
                                      C.addressof(A) if a else None, aspp, C.byref(params) if params is not None else None,
                                      out_ptr if out else None, (C.addressof(B) + (1 if misalign else 0)) if rgba else None,
                                      ws_ptr if ws else None, None)
    return rc, lib.rt_last_error().decode()


def test_every_invalid_denoise_albedo_argument_is_named_without_a_device(rt):
    P, dp = rt.DenoiseAlbedoParams, rt.denoise_albedo_params
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(s=False), "d_sum is null"), (dict(q=False), "d_sum_sq is null"), (dict(a=False), "d_albedo_sum is null"),
        (dict(out=False), "d_mean_out is null"), (dict(ws=False), "d_workspace is null"),
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(spp=1), "spp"), (dict(spp=0), "spp"), (dict(spp=-4), "spp"),
        (dict(aspp=0), "albedo_spp"), (dict(aspp=-1), "albedo_spp"),
        (dict(params=P(struct_size=12, iterations=4, sigma=4.0, eps=1e-6)), "struct_size"),
        (dict(params=P(struct_size=48, iterations=4, sigma=4.0, eps=1e-6, sigma_albedo=1.0, albedo_floor=0.1)), "struct_size"),
        (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=dp(iterations=0)), "iterations"), (dict(params=dp(iterations=7)), "iterations"),
        (dict(params=dp(sigma=0.0)), "sigma"), (dict(params=dp(sigma=nan)), "sigma"), (dict(params=dp(sigma=inf)), "sigma"),
        (dict(params=dp(eps=0.0)), "eps"), (dict(params=dp(eps=nan)), "eps"),
        (dict(params=dp(sigma_albedo=0.0)), "sigma_albedo"), (dict(params=dp(sigma_albedo=-0.5)), "sigma_albedo"),
        (dict(params=dp(sigma_albedo=nan)), "sigma_albedo"), (dict(params=dp(sigma_albedo=inf)), "sigma_albedo"),
        (dict(params=dp(albedo_floor=0.0)), "albedo_floor"), (dict(params=dp(albedo_floor=-1e-3)), "albedo_floor"),
        (dict(params=dp(albedo_floor=nan)), "albedo_floor"), (dict(params=dp(albedo_floor=inf)), "albedo_floor"),
        (dict(alias="sum"), "d_mean_out"), (dict(alias="sum_sq"), "d_mean_out"), (dict(alias="albedo"), "d_albedo_sum"),
        (dict(alias="albedo0"), "d_albedo_sum"),
        (dict(misalign=True), "d_rgba8"), (dict(ws_misalign=True), "d_workspace"),
    ]
    for kw, field in cases:
        rc, msg = _denoise(rt, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith("rt_denoise_albedo_device: "), (kw, msg)
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(rgba=False), dict(spp=1, spp_map=True), dict(spp=2, aspp=1), dict(params=dp(iterations=6)),
               dict(params=dp(iterations=1, sigma=0.5, eps=1e-12, sigma_albedo=1e-9, albedo_floor=1e-300)),
               dict(params=P(struct_size=8, iterations=2)), dict(params=P(struct_size=24, iterations=2, sigma=1.0, eps=1e-3))):
        rc, msg = _denoise(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)
    # a shorter struct's missing fields are the defaults, not the bytes behind it
    rc, msg = _denoise(rt, params=P(struct_size=24, iterations=2, sigma=1.0, eps=1e-3, sigma_albedo=0.0, albedo_floor=nan))
    assert "not a device pointer" in msg, msg


# ---- the numpy restatement ----
def _r(x):
    return float(x)  # Fraction -> the nearest double, ties to even: one correctly rounded operation


def _F(x):
    return Fraction(x)


def _exact_two_pixels(S, Q, n, A, n_a, sigma, eps, sigma_albedo, floor):
    """A 2 x 1 frame, one iteration at stride 1, in exact rational arithmetic rounded after every operation (a square root: the
    correctly rounded one of the rounded argument, checked by squaring its neighbours).  Returns out (2, 3) as floats."""
    import math
    mx = lambda a, b: b if b > a else a
    m = [[_r(_F(s) / n) for s in S[p]] for p in range(2)]
    a = [[_r(_F(x) / n_a) for x in A[p]] for p in range(2)]
    d = [[mx(x, floor) for x in a[p]] for p in range(2)]
    I = [[_r(_F(m[p][c]) / _F(d[p][c])) for c in range(3)] for p in range(2)]
    v = [[_r(_F(_r(_F(Q[p][c]) - _F(_r(_F(S[p][c]) * _F(m[p][c]))))) / (n - 1)) for c in range(3)] for p in range(2)]
    u = [[_r(_F(v[p][c]) / _F(_r(_F(d[p][c]) * _F(d[p][c])))) for c in range(3)] for p in range(2)]
    V = [_r(_F(mx(mx(mx(u[p][0], u[p][1]), u[p][2]), 0.0)) / n) for p in range(2)]
    L = [_r(_F(_r(_F(_r(_F(I[p][0]) + _F(I[p][1]))) + _F(I[p][2]))) / 3) for p in range(2)]
    out = []
    for p in range(2):
        taps = ([(-1, 0)] if p == 1 else []) + [(0, p)] + ([(1, 1)] if p == 0 else [])  # (dx, q) in the tap order: dx = -1 first
        # prefilter: row dy = 0 only (the frame is one row), g = (1/4, 1/2, 1/4) times g[1] = 1/2
        gs, ws = 0.0, 0.0
        for dx, q in taps:
            k = 0.5 * (0.25, 0.5, 0.25)[dx + 1]
            gs = _r(_F(gs) + _F(_r(_F(k) * _F(V[q]))))
            ws = _r(_F(ws) + _F(k))
        G = _r(_F(gs) / _F(ws))
        sd = math.sqrt(G)
        for cand in (np.nextafter(sd, 0.0), sd, np.nextafter(sd, np.inf)):  # math.sqrt is IEEE: its neighbours are further from the root
            assert abs(_F(float(cand)) ** 2 - _F(G)) >= abs(_F(sd) ** 2 - _F(G)) or cand == sd
        den = _r(_F(_r(_F(sigma) * _F(sd))) + _F(eps))
        sw, sv, sc = 0.0, 0.0, [0.0, 0.0, 0.0]
        for dx, q in taps:
            x = _r(abs(_F(L[p]) - _F(L[q])))
            x = _r(_F(x) / _F(den))
            t = _r(1 - _F(_r(_F(x) * _F(x))))
            e = _r(_F(t) * _F(t)) if t > 0.0 else 0.0
            da = mx(mx(_r(abs(_F(a[p][0]) - _F(a[q][0]))), _r(abs(_F(a[p][1]) - _F(a[q][1])))), _r(abs(_F(a[p][2]) - _F(a[q][2]))))
            y = _r(_F(da) / _F(sigma_albedo))
            ta = _r(1 - _F(_r(_F(y) * _F(y))))
            ea = _r(_F(ta) * _F(ta)) if ta > 0.0 else 0.0
            hh = _r(_F(dh.H5[2]) * _F(dh.H5[dx + 2]))
            wq = _r(_F(hh) * _F(_r(_F(e) * _F(ea))))
            sw = _r(_F(sw) + _F(wq))
            for c in range(3):
                sc[c] = _r(_F(sc[c]) + _F(_r(_F(wq) * _F(I[q][c]))))
            sv = _r(_F(sv) + _F(_r(_F(_r(_F(wq) * _F(wq))) * _F(V[q]))))
        C1 = [_r(_F(sc[c]) / _F(sw)) for c in range(3)]
        out.append([_r(_F(C1[c]) * _F(d[p][c])) for c in range(3)])
    return out


@pytest.mark.parametrize("floor, sigma_albedo", [(1e-3, 0.5), (0.3, 0.5), (1e-3, 0.15), (0.05, 2.0)])
def test_the_numpy_statement_is_the_definition_rounded_once_per_operation(floor, sigma_albedo):
    """Two pixels side by side with different albedos, one channel of the second below a floor of 0.3 and its difference to the
    first above a sigma_albedo of 0.15 (ea = 0 there): floor, demodulate, u, da, ea, e * ea and remodulate in exact arithmetic."""
    S = [[0.7, 2.3, 1.1], [0.9, 2.0, 1.3]]
    Q = [[0.41, 1.9, 0.52], [0.45, 1.7, 0.66]]
    A = [[1.3, 2.9, 0.8], [1.9, 2.2, 0.3]]
    n, n_a = 3, 4
    want = _exact_two_pixels(S, Q, n, A, n_a, 4.0, 1e-6, sigma_albedo, floor)
    got = ah.denoise_albedo(np.array([S]), np.array([Q]), n, np.array([A]), n_a, iterations=1, sigma_albedo=sigma_albedo, albedo_floor=floor)
    assert [[float(x).hex() for x in px] for px in got[0]] == [[x.hex() for x in px] for px in want]
    C0, V0, valid, a, d = ah.prepare(np.array([S]), np.array([Q]), n, np.array([A]), n_a, floor)
    assert valid.all() and (d >= floor).all() and ((d == floor) == (a < floor)).all()
    if floor == 0.3:
        assert (d == floor).sum() == 2      # 0.8 / 4 and 0.3 / 4
    if sigma_albedo == 0.15:
        plain_centre = ah.denoise_albedo(np.array([S])[:, :1], np.array([Q])[:, :1], n, np.array([A])[:, :1], n_a, iterations=1,
                                         sigma_albedo=sigma_albedo, albedo_floor=floor)
        assert_bits(got[:, :1], plain_centre, "ea = 0: the neighbour is no tap")


def test_pixels_that_are_not_valid_keep_their_mean_and_are_no_taps():
    S, Q, spp, spp_map = dh.synthetic(17, 9, 3)
    A, n_a = ah.synthetic_albedo(17, 9, 4)
    out = ah.denoise_albedo(S, Q, spp_map, A, n_a)
    C0, V0, valid, a, d = ah.prepare(S, Q, spp_map, A, n_a, ah.DEFAULTS["albedo_floor"])
    assert valid.any() and not valid.all() and (~np.isfinite(A)).any() and (spp_map < 2).any()
    with np.errstate(all="ignore"):
        m = S / spp_map.astype(np.float64)[:, :, None]
    assert_bits(out[~valid], m[~valid], "a pixel that is not valid is written unchanged")
    assert np.isfinite(out[valid]).all(), "a valid pixel took a tap that is not valid"
    assert (V0[~valid] == -1.0).all() and (a[valid & (d == ah.DEFAULTS["albedo_floor"]).any(axis=2)] < ah.DEFAULTS["albedo_floor"]).any()


@pytest.mark.parametrize("w, h, k", [(1, 1, 1), (5, 3, 2), (17, 9, 4), (70, 37, 4), (40, 21, 6)])
def test_an_albedo_of_one_everywhere_is_the_plain_filter_bit_for_bit(w, h, k):
    S, Q, spp, spp_map = dh.synthetic(w, h, 1000 * w + h)
    for n_a in (1, 3, 16):
        A = np.full((h, w, 3), float(n_a))
        for n in (spp, spp_map):
            assert_bits(ah.denoise_albedo(S, Q, n, A, n_a, iterations=k), dh.denoise(S, Q, n, iterations=k), f"{w}x{h}, K = {k}, n_a = {n_a}")
    assert_bits(ah.denoise_albedo(S, Q, spp, np.full((h, w, 3), 2.0), 2, iterations=k, sigma=1.5, eps=1e-3, sigma_albedo=1e-9, albedo_floor=1.0),
                dh.denoise(S, Q, spp, iterations=k, sigma=1.5, eps=1e-3), "other parameters, a floor of exactly 1")


# ---- the oracle's word on what an albedo scene's render is ----
def test_the_oracles_paths_through_an_albedo_scene_end_at_the_first_hit(rt, oracle):
    hs = scene_cases.build(rt, "ragged_cornell_37x37_4spp")
    assert hs.camera.max_depth == 8
    alb = ah.AlbedoScene(rt, hs)
    assert tuple(alb.camera.background.tuple()) == (1.0, 1.0, 1.0) and bytes(hs.desc) != bytes(alb.desc)

    class Flat:  # every lambertian the same solid
        def __init__(self):
            d = rt.SceneDesc.from_buffer_copy(hs.desc)
            self._tex = (rt.Texture * d.n_textures)(*[rt.Texture.from_buffer_copy(d.textures[t]) for t in range(d.n_textures)])
            self._mat = (rt.Material * d.n_materials)(*[rt.Material.from_buffer_copy(d.materials[k]) for k in range(d.n_materials)])
            grey = next(k for k in range(d.n_materials) if self._mat[k].kind == rt.RT_MATERIAL_LAMBERTIAN)
            for k in range(d.n_materials):
                if self._mat[k].kind == rt.RT_MATERIAL_LAMBERTIAN:
                    self._mat[k].texture = self._mat[grey].texture
            d.materials, d.textures = self._mat, self._tex
            self.desc, self.camera = d, hs.camera
    flat = ah.AlbedoScene(rt, Flat())
    for name, scene in (("the Cornell box", alb), ("its flat-colour variant", flat)):
        one = oracle.render(scene, rt.render_params(seed=9, sample_end=4, max_depth=1))
        eight = oracle.render(scene, rt.render_params(seed=9, sample_end=4, max_depth=8))
        assert_bits(one, eight, f"{name}: max_depth 1 against max_depth 8")
        assert np.isfinite(one).all() and len(np.unique(one)) > 2
    # the flat variant's albedo frame has the lambertians' one colour, the light's emission or the white of a miss in every sample
    colours = {tuple(c) for c in (oracle.render(flat, rt.render_params(seed=9, sample_end=1)).reshape(-1, 3)).tolist()}
    assert 2 <= len(colours) <= 3, colours
    # and the beauty render of the original does depend on the depth: the identity above is the albedo scene's
    assert not np.array_equal(oracle.render(hs, rt.render_params(seed=9, sample_end=4, max_depth=1)),
                              oracle.render(hs, rt.render_params(seed=9, sample_end=4, max_depth=8)))
