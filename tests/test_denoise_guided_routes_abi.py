"""The edge guide's means, spatial-variance and views forms at the C ABI without a GPU: the four symbols, their ctypes prototypes
against the header's parameter lists and their Rust declarations, the views workspace, and every invalid argument of
rt_denoise_guided_mean_device, rt_denoise_guided_mean_spatial_device and rt_denoise_guided_views_device — in the header's order, the
field named, before any device work.  The calls run on HOST buffers, as tests/test_views_denoise_abi.py runs its own: only argument
checks can answer, and past them the look-up of the device that owns d_mean_out refuses a host pointer."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_denoise_guided_mean_device", "rt_denoise_guided_mean_spatial_device", "rt_denoise_guided_views_workspace_bytes",
           "rt_denoise_guided_views_device")
MAX_VIEWS = 65535
NAN, INF = float("nan"), float("inf")


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


def test_the_symbols_are_exported_declared_and_bound_with_the_headers_prototypes(rt):
    lib = rt.amd_lib()
    text = (ROOT / "INTEGRATION.md").read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_amd.so")], check=True, capture_output=True, text=True).stdout
    ctype = {"int32_t": C.c_int32, "int": C.c_int, "int64_t": C.c_int64}
    for fn in SYMBOLS:
        assert getattr(lib, fn) is not None
        assert re.search(r" T " + fn + r"$", exported, flags=re.M), fn
        assert f"pub fn {fn}(" in text, fn
        ret, params = header_parameters(fn)
        restype, argtypes = rt.RT_AMD_SYMBOLS[fn]
        assert restype is ctype[ret], fn
        assert list(argtypes) == [C.c_void_p if "*" in p else ctype[p] for p in params], (fn, params)
    assert header_parameters("rt_denoise_guided_views_device")[1][:3] == ["int32_t"] * 3, "n_views comes behind height"
    for name in ("denoise_guided_mean_device", "denoise_guided_mean_spatial_device", "denoise_guided_views_device",
                 "denoise_guided_views_workspace_bytes", "denoise_guided_mean", "denoise_guided_mean_spatial", "denoise_guided_views"):
        assert callable(getattr(rt, name)), name
    # the Python layouts the calls take are the header's (tests/test_denoise_guided_abi.py and test_denoise_spatial_abi.py hold them to gcc)
    assert C.sizeof(rt.DenoiseGuidedParams) == 48 and C.sizeof(rt.DenoiseSpatialParams) == 12
    assert [f for f, _ in rt.DenoiseGuidedParams._fields_] == ["struct_size", "iterations", "sigma", "eps", "sigma_albedo", "albedo_floor", "sigma_edge"]
    header = (ROOT / "include" / "rt_amd.h").read_text()
    assert "views forms have no edge guide" not in header, "the sentence that said these forms do not exist"


def test_the_views_workspace_is_n_views_times_the_single_frames(rt):
    lib = rt.amd_lib()
    for w, h in ((1, 1), (33, 9), (32, 8), (70, 19), (256, 256)):
        for n in (1, 2, 5, 24, MAX_VIEWS):
            for with_albedo in (0, 1, 7):
                one = lib.rt_denoise_guided_workspace_bytes(w, h, with_albedo)
                assert lib.rt_denoise_guided_views_workspace_bytes(w, h, n, with_albedo) == n * one == n * (4 if with_albedo else 3) * 32 * w * h
                assert rt.denoise_guided_views_workspace_bytes(w, h, n, with_albedo) == n * rt.denoise_guided_workspace_bytes(w, h, with_albedo)
    # what the call refuses: a frame of 2^27 pixels or more, an empty one, fewer than one view, more views than the grid carries; and a
    # product that does not fit an int64 ((2^27 - 1) pixels x 96 bytes x (2^31 - 1) views is about 2^64.6)
    refused = [(1 << 14, 1 << 13, 1), (1 << 27, 1, 2), (0, 4, 1), (4, 0, 1), (-1, 4, 1), (4, 4, 0), (4, 4, -1), (4, 4, -(1 << 31)),
               (4, 4, MAX_VIEWS + 1), ((1 << 27) - 1, 1, (1 << 31) - 1), (1 << 13, (1 << 14) - 1, (1 << 31) - 1)]
    for w, h, n in refused:
        for with_albedo in (0, 1):
            assert lib.rt_denoise_guided_views_workspace_bytes(w, h, n, with_albedo) == -1, (w, h, n)
            with pytest.raises(rt.RtError):
                rt.denoise_guided_views_workspace_bytes(w, h, n, with_albedo)


def _call(rt, form, *, w=6, h=4, n_views=3, first=True, second=True, a=True, e=True, n=8, albedo_spp=4, edge_spp=4, spatial=None, params=None,
          out=True, rgba=True, ws=True, alias=None, misalign=False, ws_misalign=False, buffers=None):
    """One call of the `form` ("mean", "spatial", "views") entry point on HOST buffers sized for `buffers` views (1 off the views form)."""
    lib = rt.amd_lib()
    v = buffers if buffers is not None else (max(n_views, 1) if form == "views" else 1)
    px = w * h if w > 0 and h > 0 else 1
    frame = 3 * px * v
    S, Q, A, E, M = ((C.c_double * frame)() for _ in range(5))
    B = (C.c_uint8 * (4 * px * v + 4))()
    W = (C.c_uint8 * (128 * px * v + 32))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    out_ptr = C.addressof(M)
    if alias is not None:
        src, view = alias  # d_mean_out begins at the last double of `view` of that input: only a whole-extent test sees views > 0
        out_ptr = C.addressof({"first": S, "second": Q, "albedo": A, "edge": E}[src]) + 8 * (3 * px * (view + 1) - 1)
    p = lambda buf, on: C.addressof(buf) if on else None  # noqa: E731
    tail = (C.byref(params) if params is not None else None, out_ptr if out else None, (C.addressof(B) + (1 if misalign else 0)) if rgba else None,
            ws_ptr if ws else None, None)
    if form == "mean":
        rc = lib.rt_denoise_guided_mean_device(w, h, p(S, first), p(Q, second), n, p(A, a), p(E, e), *tail)
    elif form == "spatial":
        rc = lib.rt_denoise_guided_mean_spatial_device(w, h, p(S, first), p(Q, second), n, p(A, a), p(E, e),
                                                       C.byref(spatial) if spatial is not None else None, *tail)
    else:
        rc = lib.rt_denoise_guided_views_device(w, h, n_views, p(S, first), p(Q, second), n, p(A, a), albedo_spp, p(E, e), edge_spp, *tail)
    return rc, lib.rt_last_error().decode()


WHO = {"mean": "rt_denoise_guided_mean_device: ", "spatial": "rt_denoise_guided_mean_spatial_device: ", "views": "rt_denoise_guided_views_device: "}
NAMES = {"mean": ("d_mean", "d_m2", "d_albedo_mean", "d_edge_mean"), "spatial": ("d_mean", "d_m2", "d_albedo_mean", "d_edge_mean"),
         "views": ("d_sum", "d_sum_sq", "d_albedo_sum", "d_edge_sum")}


@pytest.mark.parametrize("with_albedo", [False, True])
@pytest.mark.parametrize("form", ["mean", "spatial", "views"])
def test_every_invalid_argument_is_named_without_a_device(rt, form, with_albedo):
    P, make = rt.DenoiseGuidedParams, rt.denoise_guided_params
    first, second, third, fourth = NAMES[form]
    count = "spp" if form == "views" else "samples"
    base = dict(a=with_albedo)
    cases = [
        (dict(first=False), first + " is null"), (dict(e=False), fourth + " is null"), (dict(out=False), "d_mean_out is null"),
        (dict(ws=False), "d_workspace is null"),
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13, buffers=0), "2^27"),
        (dict(n=0), count), (dict(n=-4), count),
        (dict(params=P(struct_size=12, iterations=4, sigma=4.0, eps=1e-6)), "rt_denoise_guided_params.struct_size"),
        (dict(params=P(struct_size=C.sizeof(P) + 8, iterations=4, sigma=4.0, eps=1e-6)), "rt_denoise_guided_params.struct_size"),
        (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=make(iterations=0)), "iterations"), (dict(params=make(iterations=7)), "iterations"),
        (dict(params=make(sigma=0.0)), "sigma"), (dict(params=make(sigma=NAN)), "sigma"), (dict(params=make(eps=0.0)), "eps"),
        (dict(params=make(eps=INF)), "eps"),
        (dict(params=make(sigma_edge=0.0)), "sigma_edge"), (dict(params=make(sigma_edge=-1.0)), "sigma_edge"),
        (dict(params=make(sigma_edge=NAN)), "sigma_edge"), (dict(params=make(sigma_edge=INF)), "sigma_edge"),
        (dict(alias=("first", 0)), "d_mean_out must not overlap " + first), (dict(alias=("edge", 0)), "d_mean_out must not overlap " + fourth),
        (dict(misalign=True), "d_rgba8"), (dict(ws_misalign=True), "d_workspace"),
    ]
    if form != "spatial":
        cases += [(dict(second=False), second + " is null"), (dict(alias=("second", 0)), "d_mean_out must not overlap")]
    if form == "views":
        cases += [(dict(n=1), "spp"), (dict(edge_spp=0), "edge_spp"), (dict(edge_spp=-3), "edge_spp"),
                  (dict(n_views=0), "n_views"), (dict(n_views=-1), "n_views"), (dict(n_views=MAX_VIEWS + 1, buffers=1), "n_views"),
                  (dict(alias=("first", 2)), "d_mean_out must not overlap"), (dict(alias=("second", 1)), "d_mean_out must not overlap"),
                  (dict(alias=("edge", 1)), "d_mean_out must not overlap d_edge_sum"), (dict(alias=("edge", 2)), "d_mean_out must not overlap d_edge_sum")]
    if form == "spatial":
        S = rt.DenoiseSpatialParams
        cases += [(dict(spatial=S(struct_size=6, spatial_below=2, window_radius=1)), "rt_denoise_spatial_params.struct_size"),
                  (dict(spatial=rt.denoise_spatial_params(spatial_below=0)), "spatial_below"),
                  (dict(spatial=rt.denoise_spatial_params(window_radius=0)), "window_radius"),
                  (dict(spatial=rt.denoise_spatial_params(window_radius=4)), "window_radius"),
                  (dict(second=False, n=2), "d_m2 is null"), (dict(second=False, n=1, spatial=rt.denoise_spatial_params(spatial_below=1)), "d_m2 is null"),
                  (dict(alias=("second", 0), n=2), "d_mean_out must not overlap")]
    if with_albedo:
        cases += [(dict(params=make(sigma_albedo=0.0)), "sigma_albedo"), (dict(params=make(sigma_albedo=NAN)), "sigma_albedo"),
                  (dict(params=make(albedo_floor=0.0)), "albedo_floor"), (dict(params=make(albedo_floor=INF)), "albedo_floor"),
                  (dict(alias=("albedo", 0)), "d_mean_out must not overlap")]
        if form == "views":
            cases += [(dict(albedo_spp=0), "albedo_spp"), (dict(alias=("albedo", 2)), "d_mean_out must not overlap")]
    for kw, field in cases:
        rc, msg = _call(rt, form, **{**base, **kw})
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith(WHO[form]), (kw, msg)
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    fine = [dict(), dict(rgba=False), dict(params=make(iterations=6)), dict(params=P(struct_size=8, iterations=2)), dict(n=2)]
    if not with_albedo:  # without an albedo frame its fields and its count are not read
        fine += [dict(params=make(sigma_albedo=NAN, albedo_floor=-1.0)), dict(albedo_spp=0)]
    if form != "views":
        fine += [dict(n=1), dict(edge_spp=0)]
    if form == "spatial":
        fine += [dict(second=False, n=1), dict(second=False, n=3, spatial=rt.denoise_spatial_params(spatial_below=4, window_radius=3))]
    if form == "views":
        fine += [dict(n_views=1), dict(n_views=MAX_VIEWS, w=1, h=1)]
    for kw in fine:
        rc, msg = _call(rt, form, **{**base, **kw})
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)


@pytest.mark.parametrize("form", ["mean", "spatial", "views"])
def test_the_refusals_come_in_the_headers_order(rt, form):
    """Each call below breaks two or more rules; the message names the one the header lists first."""
    make = rt.denoise_guided_params
    first, second, third, fourth = NAMES[form]
    bad_all = make(iterations=0, sigma=0.0, eps=0.0, sigma_albedo=0.0, albedo_floor=0.0, sigma_edge=0.0)
    ladder = [  # each entry adds the violation that must win over everything behind it
        (dict(misalign=True, ws_misalign=True), "d_rgba8"),
        (dict(alias=("edge", 0)), "d_mean_out must not overlap " + fourth),
        (dict(alias=("first", 0)), "d_mean_out must not overlap " + first),
    ]
    kw = {}
    for add, field in ladder:
        kw = {**kw, **add}
        rc, msg = _call(rt, form, **kw)
        assert rc == -1 and field in msg, (form, kw, msg)
    # (an alias is one pointer: the two overlap rules are told apart by which input d_mean_out lies in)
    rc, msg = _call(rt, form, alias=("edge", 0), params=make(sigma_edge=0.0))
    assert "sigma_edge" in msg, msg
    for fields, field in ((dict(sigma_edge=0.0, albedo_floor=0.0), "albedo_floor"), (dict(albedo_floor=0.0, sigma_albedo=0.0), "sigma_albedo"),
                          (dict(sigma_albedo=0.0, eps=0.0), "eps"), (dict(eps=0.0, sigma=0.0), "sigma must"), (dict(sigma=0.0, iterations=0), "iterations")):
        rc, msg = _call(rt, form, params=make(**fields))
        assert rc == -1 and field in msg, (form, fields, msg)
    bad_all.struct_size = 12
    rc, msg = _call(rt, form, params=bad_all)
    assert "rt_denoise_guided_params.struct_size" in msg, msg
    if form == "spatial":
        S = rt.DenoiseSpatialParams
        rc, msg = _call(rt, form, params=bad_all, second=False, n=2, spatial=rt.denoise_spatial_params(window_radius=9))
        assert "window_radius" in msg, msg
        rc, msg = _call(rt, form, spatial=S(struct_size=12, spatial_below=0, window_radius=9))
        assert "spatial_below" in msg, msg
        rc, msg = _call(rt, form, spatial=S(struct_size=5, spatial_below=0, window_radius=9))
        assert "rt_denoise_spatial_params.struct_size" in msg, msg
        rc, msg = _call(rt, form, n=0, spatial=S(struct_size=5, spatial_below=0, window_radius=9))
        assert "samples" in msg, msg
    if form == "views":
        rc, msg = _call(rt, form, edge_spp=0, params=bad_all)
        assert "edge_spp" in msg, msg
        rc, msg = _call(rt, form, edge_spp=0, albedo_spp=0)
        assert "albedo_spp" in msg, msg
        rc, msg = _call(rt, form, n=1, albedo_spp=0, edge_spp=0)
        assert "spp must be at least 2" in msg, msg
    count_bad = dict(n=1) if form == "views" else dict(n=0)
    rc, msg = _call(rt, form, ws=False, **count_bad)
    assert "d_workspace is null" in msg, msg
    rc, msg = _call(rt, form, ws=False, out=False)
    assert "d_mean_out is null" in msg, msg
    rc, msg = _call(rt, form, out=False, e=False)
    assert fourth + " is null" in msg, msg
    if form != "spatial":
        rc, msg = _call(rt, form, e=False, second=False)
        assert second + " is null" in msg, msg
    rc, msg = _call(rt, form, e=False, second=False, first=False)
    assert first + " is null" in msg, msg
    if form == "views":
        rc, msg = _call(rt, form, first=False, n_views=0)
        assert "n_views" in msg, msg
    rc, msg = _call(rt, form, first=False, n_views=0, w=0)
    assert "width" in msg, msg
