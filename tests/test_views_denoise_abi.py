"""The views moments and the views denoisers' C ABI without a GPU: the six symbols, their ctypes prototypes against the header's
parameter lists and their Rust declarations, the workspace sizes, and every invalid argument of rt_denoise_views_device,
rt_denoise_albedo_views_device and rt_render_views_moments[_device] — checked before any device work, the field named.  The calls
run on HOST buffers, as tests/test_denoise_abi.py runs the single-frame ones: only argument checks can answer."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_render_views_moments_device", "rt_render_views_moments", "rt_denoise_views_workspace_bytes",
           "rt_denoise_albedo_views_workspace_bytes", "rt_denoise_views_device", "rt_denoise_albedo_views_device")
MAX_VIEWS = 65535


def header_parameters(fn):
    """the C types of fn's parameters in include/rt_amd.h, comments dropped: ['int32_t', 'const double *', ...]"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rt_amd.h").read_text(), flags=re.S)
    m = re.search(r"\b(int|int64_t) " + fn + r"\(([^)]*)\)\s*;", text)
    assert m, fn
    types = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        types.append(re.sub(r"\s*\w+$", "", p) if not p.endswith("*") else p)
    return m.group(1), types


def ctype_of(c_type):
    if c_type.endswith("*"):
        return {"const rt_view *": "POINTER(View)", "const rt_render_params *": "POINTER(RenderParams)"}.get(c_type, "c_void_p")
    return {"int32_t": "c_int32", "int": "c_int", "int64_t": "c_int64"}[c_type]


def test_the_symbols_are_exported_declared_and_bound_with_the_headers_prototypes(rt):
    lib = rt.amd_lib()
    text = (ROOT / "INTEGRATION.md").read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_amd.so")], check=True, capture_output=True, text=True).stdout
    names = {"POINTER(View)": C.POINTER(rt.View), "POINTER(RenderParams)": C.POINTER(rt.RenderParams), "c_void_p": C.c_void_p,
             "c_int32": C.c_int32, "c_int": C.c_int, "c_int64": C.c_int64}
    for fn in SYMBOLS:
        assert getattr(lib, fn) is not None
        assert re.search(r" T " + fn + r"$", exported, flags=re.M), fn
        assert f"pub fn {fn}(" in text, fn
        ret, params = header_parameters(fn)
        restype, argtypes = rt.RT_AMD_SYMBOLS[fn]
        assert restype is names[ctype_of(ret)], fn
        assert list(argtypes) == [names[ctype_of(p)] for p in params], (fn, params)
    assert header_parameters("rt_denoise_views_device")[1][:3] == ["int32_t"] * 3, "n_views comes behind height"
    assert re.search(r"#define RT_DENOISE_MAX_VIEWS " + str(MAX_VIEWS) + r"\b", (ROOT / "include" / "rt_amd.h").read_text())
    for name in ("render_views_moments", "render_views_moments_device"):
        assert callable(getattr(rt.DeviceScene, name))
    for name in ("denoise_views_workspace_bytes", "denoise_albedo_views_workspace_bytes", "denoise_views_device", "denoise_albedo_views_device",
                 "denoise_views", "denoise_albedo_views"):
        assert callable(getattr(rt, name)), name


def test_the_workspaces_are_n_views_times_the_single_frames(rt):
    lib = rt.amd_lib()
    for w, h in ((1, 1), (33, 9), (32, 8), (70, 19), (256, 256), (400, 225)):
        for n in (1, 2, 5, 24, MAX_VIEWS):
            assert lib.rt_denoise_views_workspace_bytes(w, h, n) == n * lib.rt_denoise_workspace_bytes(w, h) == n * 2 * 32 * w * h
            assert lib.rt_denoise_albedo_views_workspace_bytes(w, h, n) == n * lib.rt_denoise_albedo_workspace_bytes(w, h) == n * 3 * 32 * w * h
            assert rt.denoise_views_workspace_bytes(w, h, n) == n * rt.denoise_workspace_bytes(w, h)
            assert rt.denoise_albedo_views_workspace_bytes(w, h, n) == n * rt.denoise_albedo_workspace_bytes(w, h)
    # what the call would refuse: a frame of 2^27 pixels or more, an empty one, fewer than one view, more views than the grid carries;
    # and a product that does not fit an int64 ((2^27 - 1) pixels x 96 bytes x (2^31 - 1) views is about 2^64.6)
    refused = [(1 << 14, 1 << 13, 1), (1 << 27, 1, 2), (0, 4, 1), (4, 0, 1), (-1, 4, 1), (4, 4, 0), (4, 4, -1), (4, 4, -(1 << 31)),
               (4, 4, MAX_VIEWS + 1), ((1 << 27) - 1, 1, (1 << 31) - 1), (1 << 13, (1 << 14) - 1, (1 << 31) - 1)]
    for w, h, n in refused:
        assert lib.rt_denoise_views_workspace_bytes(w, h, n) == -1, (w, h, n)
        assert lib.rt_denoise_albedo_views_workspace_bytes(w, h, n) == -1, (w, h, n)
        with pytest.raises(rt.RtError):
            rt.denoise_views_workspace_bytes(w, h, n)
        with pytest.raises(rt.RtError):
            rt.denoise_albedo_views_workspace_bytes(w, h, n)


def _denoise_views(rt, guided, *, w=6, h=4, n_views=3, s=True, q=True, a=True, spp=8, albedo_spp=4, params=None, out=True, rgba=True, ws=True,
                   alias=None, misalign=False, ws_misalign=False, buffers=None):
    """One call of rt_denoise_views_device / rt_denoise_albedo_views_device on HOST buffers (sized for `buffers` views, n_views if not
    given): past the argument checks the first thing asks the HIP runtime which device owns d_mean_out, and host memory has none."""
    lib = rt.amd_lib()
    v = buffers if buffers is not None else max(n_views, 1)
    n = w * h if w > 0 and h > 0 else 1
    frame = 3 * n * v
    S, Q, A = (C.c_double * frame)(), (C.c_double * frame)(), (C.c_double * frame)()
    # d_mean_out sits in ONE allocation directly behind a frame-sized gap, so that aliases are exact byte distances
    B = (C.c_uint8 * (4 * n * v + 4))()
    W = (C.c_uint8 * (96 * n * v + 32))()
    M = (C.c_double * frame)()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    out_ptr = C.addressof(M)
    if alias is not None:
        src, view = alias  # d_mean_out's FIRST frame begins at the last double of `view` of that input: only the whole-extent test sees it
        base = {"sum": S, "sum_sq": Q, "albedo_sum": A}[src]
        out_ptr = C.addressof(base) + 8 * (3 * n * (view + 1) - 1)
    common = (C.byref(params) if params is not None else None, out_ptr if out else None, (C.addressof(B) + (1 if misalign else 0)) if rgba else None,
              ws_ptr if ws else None, None)
    if guided:
        rc = lib.rt_denoise_albedo_views_device(w, h, n_views, C.addressof(S) if s else None, C.addressof(Q) if q else None, spp,
                                                C.addressof(A) if a else None, albedo_spp, *common)
    else:
        rc = lib.rt_denoise_views_device(w, h, n_views, C.addressof(S) if s else None, C.addressof(Q) if q else None, spp, *common)
    return rc, lib.rt_last_error().decode()


@pytest.mark.parametrize("guided", [False, True])
def test_every_invalid_views_denoise_argument_is_named_without_a_device(rt, guided):
    P = rt.DenoiseAlbedoParams if guided else rt.DenoiseParams
    make = rt.denoise_albedo_params if guided else rt.denoise_params
    who = "rt_denoise_albedo_views_device: " if guided else "rt_denoise_views_device: "
    nan, inf = float("nan"), float("inf")
    cases = [
        # the single-frame refusals
        (dict(s=False), "d_sum is null"), (dict(q=False), "d_sum_sq is null"), (dict(out=False), "d_mean_out is null"),
        (dict(ws=False), "d_workspace is null"),
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13, buffers=0), "2^27"),
        (dict(spp=1), "spp"), (dict(spp=0), "spp"), (dict(spp=-4), "spp"),
        (dict(params=P(struct_size=12, iterations=4, sigma=4.0, eps=1e-6)), "struct_size"),
        (dict(params=P(struct_size=C.sizeof(P) + 8, iterations=4, sigma=4.0, eps=1e-6)), "struct_size"),
        (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=make(iterations=0)), "iterations"), (dict(params=make(iterations=7)), "iterations"),
        (dict(params=make(sigma=0.0)), "sigma"), (dict(params=make(sigma=nan)), "sigma"), (dict(params=make(sigma=inf)), "sigma"),
        (dict(params=make(eps=0.0)), "eps"), (dict(params=make(eps=nan)), "eps"),
        (dict(misalign=True), "d_rgba8"), (dict(ws_misalign=True), "d_workspace"),
        # the stack's own
        (dict(n_views=0), "n_views"), (dict(n_views=-1), "n_views"), (dict(n_views=MAX_VIEWS + 1, buffers=1), "n_views"),
        (dict(n_views=(1 << 31) - 1, buffers=1), "n_views"),
        # d_mean_out overlapping an input anywhere in the whole extent: behind the first view, and at the last double of the last
        (dict(alias=("sum", 0)), "d_mean_out"), (dict(alias=("sum", 2)), "d_mean_out"), (dict(alias=("sum_sq", 1)), "d_mean_out"),
        (dict(alias=("sum_sq", 2)), "d_mean_out"),
    ]
    if guided:
        cases += [
            (dict(a=False), "d_albedo_sum is null"), (dict(albedo_spp=0), "albedo_spp"), (dict(albedo_spp=-2), "albedo_spp"),
            (dict(params=make(sigma_albedo=0.0)), "sigma_albedo"), (dict(params=make(sigma_albedo=nan)), "sigma_albedo"),
            (dict(params=make(albedo_floor=0.0)), "albedo_floor"), (dict(params=make(albedo_floor=inf)), "albedo_floor"),
            (dict(alias=("albedo_sum", 1)), "d_mean_out"), (dict(alias=("albedo_sum", 2)), "d_mean_out"),
        ]
    for kw, field in cases:
        rc, msg = _denoise_views(rt, guided, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith(who), (kw, msg)
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(rgba=False), dict(n_views=1), dict(spp=2), dict(params=make(iterations=6)), dict(params=P(struct_size=8, iterations=2)),
               dict(n_views=MAX_VIEWS, w=1, h=1)):
        rc, msg = _denoise_views(rt, guided, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)


@pytest.mark.parametrize("device", [False, True])
def test_every_invalid_views_moments_argument_is_named_before_any_device_work(rt, device):
    lib = rt.amd_lib()
    hs = rt.HostScene(6, width=16, spp=8, depth=4)
    n = hs.width * hs.height
    S, Q = (C.c_double * (3 * n * 2))(), (C.c_double * (3 * n * 2))()
    fake_scene = C.c_void_p(C.addressof((C.c_uint8 * 64)()))  # never dereferenced: every case below is refused by a check before it
    who = "rt_render_views_moments_device: " if device else "rt_render_views_moments: "

    def two():
        return rt.orbit_views(hs, 2, 1)

    def call(*, scene=fake_scene, views=None, n_views=2, params=None, s=True, q=True):
        v = two() if views is None else views
        p = params if params is not None else rt.render_params(seed=1)
        args = [scene, v if v is not False else None, n_views, C.byref(p) if p is not False else None, C.addressof(S) if s else None,
                C.addressof(Q) if q else None]
        rc = lib.rt_render_views_moments_device(*args, None) if device else lib.rt_render_views_moments(*args)
        return rc, lib.rt_last_error().decode()

    wider = two()
    wider[1].camera.image_width += 8
    taller = two()
    taller[1].camera.image_height += 8
    more = two()
    more[1].camera.samples_per_pixel += 1
    cases = [
        (dict(scene=None), "scene"), (dict(views=False), "views"), (dict(params=False), "params"),
        (dict(s=False), "d_sum is null" if device else "sum is null"),
        (dict(q=False), "d_sum_sq is null" if device else "sum_sq is null"),
        (dict(n_views=0), "n_views"), (dict(n_views=-3), "n_views"),
        (dict(params=rt.render_params(shard_count=2)), "shard_count"),
        (dict(params=rt.render_params(out_layout=rt.RT_OUT_TILES)), "out_layout"),
        (dict(views=wider), "image_width"), (dict(views=taller), "image_height"),
        (dict(views=more, params=rt.render_params(sample_end=0)), "samples_per_pixel"),
    ]
    for kw, field in cases:
        rc, msg = call(**kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith(who), (kw, msg)
    # more tiles than the job index holds: RT_ERR_UNSUPPORTED, as rt_render_views_device gives it, before the views beyond the first are read
    rc, msg = call(views=rt.orbit_views(hs, 1, 1), n_views=1 << 26)
    assert rc == -5 and "n_views" in msg and msg.startswith(who), (rc, msg)
