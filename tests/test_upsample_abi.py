"""Guided upsampling's C ABI without a GPU: the symbols and their Rust declarations, the layout and the sized initialiser of
rt_upsample_params, the workspace size, every invalid argument of rt_upsample_device in the header's order (checked before any device
work, the field named), the host mirror's same refusals, and rt_camera_scaled bit for bit against its restatement."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

import upsample_helpers as uh

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_camera_scaled", "rt_upsample_params_init_sized", "rt_upsample_workspace_bytes", "rt_upsample_device")
TITLE = "guided upsampling (opt-in; nothing above changes)"


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
    assert "pub struct rt_upsample_params" in text
    order = [header.index(t) for t in ("views denoise: one filter over a stack of frames", TITLE, "bloom (opt-in; nothing above changes)",
                                       "tone mapping (opt-in; nothing above changes)")]
    assert order == sorted(order), "upsampling runs behind the denoisers and before bloom and the tone mapper"
    assert re.search(r"#define RT_ABI_VERSION 2\b", header)
    debug_header = (ROOT / "include" / "rt_amd_debug.h").read_text()
    assert "rt_debug_set_upsample_form" in rt.RT_AMD_DEBUG_SYMBOLS and re.search(r"\bint rt_debug_set_upsample_form\(", debug_header)
    assert re.search(r" T rt_debug_set_upsample_form$", exported, flags=re.M)
    host_header = (ROOT / "include" / "rt_host.h").read_text()
    host_exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_host.so")], check=True, capture_output=True, text=True).stdout
    assert "rth_upsample" in rt.RT_HOST_SYMBOLS and re.search(r"\bint rth_upsample\(", host_header) and re.search(r" T rth_upsample$", host_exported, flags=re.M)
    for name in ("upsample_params", "camera_scaled", "upsample_workspace_bytes", "upsample_device", "upsample", "upsample_host"):
        assert callable(getattr(rt, name)), name


def test_rt_upsample_params_has_gccs_layout_and_its_rust_fields(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){", 'printf("size %zu\\n", sizeof(rt_upsample_params));']
    for fname, _ in rt.UpsampleParams._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rt_upsample_params, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(rt.UpsampleParams) == 32
    for fname, _ in rt.UpsampleParams._fields_:
        assert int(got[fname]) == getattr(rt.UpsampleParams, fname).offset, fname
    text = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"pub struct rt_upsample_params\s*\{(.*?)\}", text, flags=re.S)
    assert re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in rt.UpsampleParams._fields_]


def test_init_sized_writes_the_defaults_into_struct_size_bytes_only(rt):
    lib = rt.amd_lib()
    u = rt.upsample_params()
    assert (u.struct_size, u.factor, u.sigma_edge, u.sigma_albedo, u.albedo_floor) == (32, 2, 0.5, 0.5, 1e-3)
    assert uh.DEFAULTS == dict(factor=u.factor, sigma_edge=u.sigma_edge, sigma_albedo=u.sigma_albedo, albedo_floor=u.albedo_floor)
    for size in (8, 16, 24, 32):
        buf = (C.c_uint8 * 48)(*([0xA5] * 48))
        assert lib.rt_upsample_params_init_sized(buf, size) == 0
        raw = bytes(buf)
        assert raw[size:] == b"\xa5" * (48 - size), size
        assert raw[:size] == bytes(rt.UpsampleParams(struct_size=size, factor=2, sigma_edge=0.5, sigma_albedo=0.5, albedo_floor=1e-3))[:size], size
    for size in (0, 4, 12, 20, 28, 33, 40):
        buf = (C.c_uint8 * 48)(*([0xA5] * 48))
        assert lib.rt_upsample_params_init_sized(buf, size) == -1, size
        assert "struct_size" in lib.rt_last_error().decode()
        assert bytes(buf) == b"\xa5" * 48
    assert lib.rt_upsample_params_init_sized(None, 32) == -1
    with pytest.raises(TypeError):
        rt.upsample_params(radius=3)


def test_the_workspace_is_three_regions_of_four_doubles_per_low_pixel(rt):
    lib = rt.amd_lib()
    for w, h in ((1, 1), (2, 2), (13, 7), (5, 3), (65, 17), (1200, 800), (1 << 13, 1 << 13), ((1 << 27) - 1, 1)):
        for F in uh.FACTORS:
            want = 3 * 32 * uh.low_size(w, F) * uh.low_size(h, F)
            assert lib.rt_upsample_workspace_bytes(w, h, F) == want == rt.upsample_workspace_bytes(w, h, F), (w, h, F)
            assert want % 16 == 0
    assert lib.rt_upsample_workspace_bytes(13, 7, 2) == 96 * 7 * 4
    for w, h, F in ((0, 4, 2), (4, 0, 2), (-1, 4, 2), (1 << 14, 1 << 13, 2), (1 << 27, 1, 4), (8, 8, 1), (8, 8, 5), (8, 8, 0), (8, 8, -2)):
        assert lib.rt_upsample_workspace_bytes(w, h, F) == -1, (w, h, F)
        with pytest.raises(rt.RtError):
            rt.upsample_workspace_bytes(w, h, F)


def _upsample(rt, *, w=6, h=4, low=True, out=True, ws=True, spp=8, albedo=False, albedo_spp=0, edge=False, edge_spp=0, params=None,
              rgba_misalign=False, ws_misalign=False, alias=None):
    """One call of rt_upsample_device on HOST buffers: only argument checks can answer (the first thing past them asks the HIP runtime
    which device owns the output, and host memory has none)."""
    lib = rt.amd_lib()
    n = w * h if w > 0 and h > 0 and w * h < 1 << 20 else 1
    arena = (C.c_double * (13 * 3 * n))()   # the four frames three frames apart, so that an aliased output overlaps the one input meant
    L, A, E, O = ((C.c_double * (3 * n)).from_buffer(arena, 8 * 3 * n * k) for k in (2, 5, 8, 11))
    B = (C.c_uint8 * (4 * n + 8))()
    W = (C.c_uint8 * (96 * n + 64))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    rgba_ptr = (C.addressof(B) + 3) // 4 * 4 + (1 if rgba_misalign else 0)
    out_ptr = C.addressof(O)
    if alias == "low":       # the first double of the low frame (the frame is smaller than the output)
        out_ptr = C.addressof(L) - 8 * (3 * n - 1)
    elif alias == "albedo":  # the last double of the guide
        out_ptr = C.addressof(A) + 8 * (3 * n - 1)
    elif alias == "edge":
        out_ptr = C.addressof(E) + 8 * (3 * n - 1)
    rc = lib.rt_upsample_device(w, h, C.addressof(L) if low else None, spp, C.addressof(A) if albedo else None, albedo_spp,
                                C.addressof(E) if edge else None, edge_spp, C.byref(params) if params is not None else None,
                                out_ptr if out else None, rgba_ptr, ws_ptr if ws else None, None)
    return rc, lib.rt_last_error().decode()


def test_every_invalid_argument_is_named_without_a_device_in_the_headers_order(rt):
    P = rt.UpsampleParams
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(low=False), "d_low is null"), (dict(out=False), "d_mean_out is null"), (dict(ws=False), "d_workspace is null"),
        (dict(spp=0), "spp"), (dict(spp=-4), "spp"),
        (dict(albedo=True, albedo_spp=0), "albedo_spp"), (dict(albedo=True, albedo_spp=-1, edge=True, edge_spp=1), "albedo_spp"),
        (dict(edge=True, edge_spp=0), "edge_spp"), (dict(albedo=True, albedo_spp=1, edge=True, edge_spp=-2), "edge_spp"),
        (dict(params=P(struct_size=12)), "struct_size"), (dict(params=P(struct_size=40)), "struct_size"), (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=rt.upsample_params(factor=1)), "factor"), (dict(params=rt.upsample_params(factor=5)), "factor"),
        (dict(params=rt.upsample_params(factor=0)), "factor"), (dict(params=rt.upsample_params(factor=-2)), "factor"),
        (dict(params=rt.upsample_params(sigma_edge=0.0)), "sigma_edge"), (dict(params=rt.upsample_params(sigma_edge=nan)), "sigma_edge"),
        (dict(params=rt.upsample_params(sigma_edge=-1.0)), "sigma_edge"),
        (dict(params=rt.upsample_params(sigma_albedo=0.0)), "sigma_albedo"), (dict(params=rt.upsample_params(sigma_albedo=nan)), "sigma_albedo"),
        (dict(params=rt.upsample_params(albedo_floor=0.0)), "albedo_floor"), (dict(params=rt.upsample_params(albedo_floor=nan)), "albedo_floor"),
        (dict(params=rt.upsample_params(albedo_floor=-inf)), "albedo_floor"),
        (dict(rgba_misalign=True), "4-byte aligned"), (dict(ws_misalign=True), "16-byte aligned"),
        (dict(alias="low"), "overlap d_low"), (dict(alias="albedo", albedo=True, albedo_spp=1), "overlap d_albedo_sum"),
        (dict(alias="edge", edge=True, edge_spp=1), "overlap d_edge_sum"),
    ]
    for kw, field in cases:
        rc, msg = _upsample(rt, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith("rt_upsample_device: "), (kw, msg)
    # the header's order: of two bad arguments the earlier one is named — each entry is bad in its own way and in every later way
    order = [(dict(w=0), "width"), (dict(low=False), "d_low"), (dict(out=False), "d_mean_out"), (dict(ws=False), "d_workspace is null"),
             (dict(spp=0), "spp must"), (dict(albedo=True, albedo_spp=0), "albedo_spp"), (dict(edge=True, edge_spp=0), "edge_spp"),
             (dict(params=P(struct_size=12, factor=9)), "struct_size"), (dict(factor=9), "factor"), (dict(sigma_edge=-1.0), "sigma_edge"),
             (dict(sigma_albedo=-1.0), "sigma_albedo"), (dict(albedo_floor=-1.0), "albedo_floor"), (dict(rgba_misalign=True), "4-byte"),
             (dict(ws_misalign=True), "16-byte"), (dict(alias="low"), "overlap")]
    fields_of_params = ("factor", "sigma_edge", "sigma_albedo", "albedo_floor")
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kw, fields = {}, {}
            for extra, _ in (order[a], order[b]):
                for key, value in extra.items():
                    (fields if key in fields_of_params else kw)[key] = value
            if "ws" in kw and "ws_misalign" in kw:
                continue   # (a null workspace has no alignment)
            if "out" in kw and "alias" in kw:
                continue   # (a null output overlaps nothing)
            if "w" in kw and "alias" in kw:
                continue   # (the alias is worked out from the frame's size)
            if fields:
                if "params" in kw:
                    continue   # (an unknown struct's fields are not looked at)
                kw["params"] = rt.upsample_params(**fields)
            rc, msg = _upsample(rt, **kw)
            assert rc == -1 and order[a][1] in msg, (order[a], order[b], msg)
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(spp=1), dict(albedo=True, albedo_spp=1), dict(edge=True, edge_spp=3), dict(albedo=True, albedo_spp=2, edge=True, edge_spp=1),
               dict(albedo_spp=-5, edge_spp=-5), dict(params=rt.upsample_params(factor=4)), dict(params=P(struct_size=8, factor=3)),
               dict(params=P(struct_size=16, factor=2, sigma_edge=0.25))):
        rc, msg = _upsample(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)
    # a shorter struct's missing fields are the defaults, not the bytes behind it: albedo_floor = -1 beyond struct_size 24 is not looked at
    rc, msg = _upsample(rt, params=P(struct_size=24, factor=2, sigma_edge=0.5, sigma_albedo=0.5, albedo_floor=-1.0))
    assert "not a device pointer" in msg, msg


def test_the_host_mirror_refuses_the_same_things_with_the_same_words(rt):
    lib, host = rt.amd_lib(), rt.host_lib()
    n = 24
    L, A, O = (C.c_double * (3 * n))(), (C.c_double * (3 * n))(), (C.c_double * (3 * n))()
    W = (C.c_uint8 * (96 * n + 16))()
    ws = (C.addressof(W) + 15) // 16 * 16
    P = rt.UpsampleParams
    for kw in (dict(w=0), dict(h=0), dict(w=1 << 14, h=1 << 13), dict(spp=0), dict(albedo_spp=0), dict(params=P(struct_size=12)),
               dict(params=rt.upsample_params(factor=5)), dict(params=rt.upsample_params(sigma_edge=-1.0)),
               dict(params=rt.upsample_params(sigma_albedo=float("nan"))), dict(params=rt.upsample_params(albedo_floor=0.0)),
               dict(out=C.addressof(L) + 8), dict(out=C.addressof(A) + 8)):
        a = dict(w=6, h=4, spp=1, albedo_spp=1, params=None, out=C.addressof(O))
        a.update(kw)
        p = C.byref(a["params"]) if a["params"] is not None else None
        assert lib.rt_upsample_device(a["w"], a["h"], C.addressof(L), a["spp"], C.addressof(A), a["albedo_spp"], None, 0, p, a["out"], None, ws, None) == -1, kw
        assert host.rth_upsample(a["w"], a["h"], C.addressof(L), a["spp"], C.addressof(A), a["albedo_spp"], None, 0, p, a["out"], None) == -1, kw
        dev, mirror = lib.rt_last_error().decode(), host.rth_last_error().decode()
        assert dev.startswith("rt_upsample_device: ") and mirror.startswith("rth_upsample: ")
        tail = dev[len("rt_upsample_device: "):]
        want = tail.replace("d_mean_out", "out_mean").replace("d_low", "low").replace("d_albedo_sum", "albedo_sum").replace("d_edge_sum", "edge_sum")
        assert mirror[len("rth_upsample: "):] == want, (kw, dev, mirror)
    for name, args in (("low is null", (6, 4, None, 1, None, 0, None, 0, None, C.addressof(O), None)),
                       ("out_mean is null", (6, 4, C.addressof(L), 1, None, 0, None, 0, None, None, None))):
        assert host.rth_upsample(*args) == -1 and host.rth_last_error().decode() == "rth_upsample: " + name


def _camera(rt, w, h):
    """a camera whose vectors have full mantissas, so that a differently rounded or contracted operation shows"""
    cam = rt.Camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = w, h, 7, 11
    cam.background = rt.Vec3(0.7, 0.8, 1.0)
    cam.center = rt.Vec3(13.0, 2.0, 3.0)
    cam.pixel00_loc = rt.Vec3(-1.0 / 3.0, 2.0 / 7.0, -1.1)
    cam.pixel_delta_u = rt.Vec3(0.01 / 3.0, 1e-4 / 7.0, 0.3e-3)
    cam.pixel_delta_v = rt.Vec3(-1e-5 / 3.0, -0.013 / 7.0, 0.7e-4)
    cam.defocus_angle = 0.6
    cam.defocus_disk_u = rt.Vec3(0.1, 0.2, 0.3)
    cam.defocus_disk_v = rt.Vec3(0.4, 0.5, 0.6)
    return cam


@pytest.mark.parametrize("w,h", [(64, 64), (13, 7), (1, 1), (3, 5)], ids=lambda v: str(v))
def test_the_scaled_camera_is_the_restatements_bit_for_bit(rt, w, h):
    cam = _camera(rt, w, h)
    before = bytes(cam)
    plain = dict(w=w, h=h, p00=list(cam.pixel00_loc.tuple()), du=list(cam.pixel_delta_u.tuple()), dv=list(cam.pixel_delta_v.tuple()))
    for F in uh.FACTORS:
        got = rt.camera_scaled(cam, F)
        want = uh.camera_scaled(plain, F)
        assert (got.image_width, got.image_height) == (want["w"], want["h"]) == ((w + F - 1) // F, (h + F - 1) // F)
        assert list(got.pixel00_loc.tuple()) == want["p00"] and list(got.pixel_delta_u.tuple()) == want["du"] and list(got.pixel_delta_v.tuple()) == want["dv"]
        # the low pixel's centre is the centre of its block: pixel00' ~ pixel00 + (F - 1) / 2 * (du + dv), to rounding
        for c, (p, u, v) in enumerate(zip(plain["p00"], plain["du"], plain["dv"])):
            assert abs(want["p00"][c] - (p + (F - 1) / 2.0 * (u + v))) < 1e-15
        # everything else is untouched
        untouched = ("samples_per_pixel", "max_depth", "defocus_angle")
        assert all(getattr(got, f) == getattr(cam, f) for f in untouched)
        for f in ("background", "center", "defocus_disk_u", "defocus_disk_v"):
            assert getattr(got, f).tuple() == getattr(cam, f).tuple(), f
        assert bytes(cam) == before, "the input is not written"
    # in place is allowed
    same = rt.Camera.from_buffer_copy(cam)
    assert rt.amd_lib().rt_camera_scaled(C.byref(same), 2, C.byref(same)) == 0 and bytes(same) == bytes(rt.camera_scaled(cam, 2))


def test_the_scaled_camera_refuses_in_the_headers_order(rt):
    lib = rt.amd_lib()
    cam, out = _camera(rt, 8, 8), rt.Camera()
    for args, field in (((None, 9, None), "camera is null"), ((C.byref(cam), 9, None), "out is null"), ((C.byref(cam), 1, C.byref(out)), "factor"),
                        ((C.byref(cam), 5, C.byref(out)), "factor"), ((C.byref(cam), 0, C.byref(out)), "factor")):
        assert lib.rt_camera_scaled(*args) == -1
        msg = lib.rt_last_error().decode()
        assert msg.startswith("rt_camera_scaled: ") and field in msg, msg
    with pytest.raises(rt.RtError):
        rt.camera_scaled(cam, 7)
