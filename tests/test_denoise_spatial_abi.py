"""Spatial variance's C ABI without a GPU: the three symbols and their Rust declarations, rt_denoise_spatial_params against gcc's layout
and its sized init against a guard word, every refusal of rt_denoise_mean_spatial_device / rt_denoise_albedo_mean_spatial_device (the
field named, before a device is touched), the command line's refusals, and the numpy restatement of tests/spatial_denoise_helpers.py —
the spatial prepare, plain and guided — held to exact rational arithmetic rounded once per operation on frames of 2 x 1, 3 x 3 and
4 x 2 that reach a lone valid pixel (cnt = 1: V0 = +0.0), cnt = 2, a non-finite neighbour and the guided floor."""
import ctypes as C
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import spatial_denoise_helpers as sdh

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_denoise_spatial_params_init_sized", "rt_denoise_mean_spatial_device", "rt_denoise_albedo_mean_spatial_device")


def test_the_symbols_are_exported_declared_and_bound(rt):
    lib = rt.amd_lib()
    header = (ROOT / "include" / "rt_amd.h").read_text()
    text = (ROOT / "INTEGRATION.md").read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_amd.so")], check=True, capture_output=True, text=True).stdout
    for fn in SYMBOLS:
        assert getattr(lib, fn) is not None
        assert fn in rt.RT_AMD_SYMBOLS, fn
        assert f"int {fn}(" in header, fn
        assert f"pub fn {fn}(" in text, fn
        assert re.search(r" T " + fn + r"$", exported, flags=re.M), fn
    assert "pub struct rt_denoise_spatial_params" in text
    for name in ("denoise_spatial_params", "denoise_mean_spatial_device", "denoise_mean_spatial", "denoise_albedo_mean_spatial_device",
                 "denoise_albedo_mean_spatial"):
        assert callable(getattr(rt, name))


def test_rt_denoise_spatial_params_has_gccs_layout_and_its_rust_fields(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(rt_denoise_spatial_params));']
    for fname, _ in rt.DenoiseSpatialParams._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rt_denoise_spatial_params, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(rt.DenoiseSpatialParams) == 12
    for fname, _ in rt.DenoiseSpatialParams._fields_:
        assert int(got[fname]) == getattr(rt.DenoiseSpatialParams, fname).offset, fname
    rust = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"pub struct rt_denoise_spatial_params\s*\{(.*?)\}", rust, flags=re.S)
    assert m and re.findall(r"pub (\w+)\s*:", m.group(1)) == [f for f, _ in rt.DenoiseSpatialParams._fields_]
    # the existing params structs have not grown
    assert C.sizeof(rt.DenoiseParams) == 24 and C.sizeof(rt.DenoiseAlbedoParams) == 40


def test_the_sized_init_writes_the_defaults_into_exactly_struct_size_bytes(rt):
    lib = rt.amd_lib()
    d = rt.denoise_spatial_params()
    assert (d.struct_size, d.spatial_below, d.window_radius) == (12, 2, 1)
    assert (d.spatial_below, d.window_radius) == (sdh.DEFAULTS["spatial_below"], sdh.DEFAULTS["window_radius"])

    class Guarded(C.Structure):
        _fields_ = [("p", rt.DenoiseSpatialParams), ("guard", C.c_uint32)]

    for size in (8, 12):
        g = Guarded()
        C.memset(C.addressof(g), 0xAB, C.sizeof(g))
        assert lib.rt_denoise_spatial_params_init_sized(C.addressof(g), size) == 0
        raw = bytes(g)
        assert raw[size:] == b"\xab" * (C.sizeof(g) - size), f"the sized init wrote past the caller's {size} bytes"
        assert g.p.struct_size == size and g.p.spatial_below == 2
        assert g.guard == 0xABABABAB
        if size == 12:
            assert g.p.window_radius == 1
    for bad in (0, 4, 10, 16, 4096):
        g = Guarded()
        assert lib.rt_denoise_spatial_params_init_sized(C.addressof(g), bad) == -1 and "struct_size" in lib.rt_last_error().decode(), bad
    assert lib.rt_denoise_spatial_params_init_sized(None, 12) == -1
    with pytest.raises(TypeError):
        rt.denoise_spatial_params(sigma=1.0)


# ---- the restatement against exact rational arithmetic ----
def _r(x):
    return float(x)  # Fraction -> the nearest double, ties to even: one correctly rounded operation


def _hex(a):
    return [float(x).hex() for x in np.asarray(a).reshape(-1)]


def _max(a, b):
    return b if b > a else a


def _exact_v0(C0, valid, y, x, R):
    """V0 of the valid pixel (y, x): the definition with every operation an exact rational one rounded once"""
    h, w = valid.shape
    members = [(y + dy, x + dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)
               if 0 <= y + dy < h and 0 <= x + dx < w and valid[y + dy, x + dx]]
    cnt = float(len(members))
    v = []
    for c in range(3):
        s1 = 0.0
        for q in members:
            s1 = _r(Fraction(s1) + Fraction(float(C0[q][c])))
        mu = _r(Fraction(s1) / Fraction(cnt))
        s2 = 0.0
        for q in members:
            t = _r(Fraction(float(C0[q][c])) - Fraction(mu))
            tt = _r(Fraction(t) * Fraction(t))
            s2 = _r(Fraction(s2) + Fraction(tt))
        v.append(_r(Fraction(s2) / Fraction(cnt - 1.0)) if cnt >= 2.0 else 0.0)
    return _max(_max(v[0], v[1]), v[2]), len(members)


def _frames():
    """name -> (M, A, floor): 2 x 1 with one pixel not valid (cnt = 1), 2 x 1 whole (cnt = 2), 3 x 3 with a NaN and an inf neighbour,
    4 x 2 with albedos at, below and above the floor and one non-finite albedo"""
    rng = np.random.default_rng(11)
    out = {}
    M = rng.random((1, 2, 3)); M[0, 1, 2] = np.inf
    out["2x1 lone"] = (M, np.full((1, 2, 3), 0.5), 1e-3)
    out["2x1 pair"] = (rng.random((1, 2, 3)) * 3.0, rng.random((1, 2, 3)), 1e-3)
    M = rng.random((3, 3, 3)) * (10.0 ** rng.integers(-3, 3, size=(3, 3, 3))); M[0, 1, 0] = np.nan; M[2, 2, 1] = -np.inf
    out["3x3 holes"] = (M, rng.random((3, 3, 3)), 1e-3)
    M = rng.random((2, 4, 3))
    A = rng.random((2, 4, 3)); A[0, 0] = (0.0, 1e-5, 1.75); A[0, 1] = (1e-3, 5e-4, 0.3); A[1, 2, 1] = np.nan; A[1, 3] = (1e-9, 2.0, 0.05)
    out["4x2 floor"] = (M, A, 1e-3)
    out["4x2 high floor"] = (M, A, 0.25)
    return out


@pytest.mark.parametrize("name", list(_frames()))
@pytest.mark.parametrize("R", [1, 2, 3])
def test_the_spatial_prepare_is_the_definition_rounded_once_per_operation(name, R):
    M, A, floor = _frames()[name]
    h, w = M.shape[:2]
    C0, V0, valid = sdh.prepare_spatial(M, R)
    assert valid.tolist() == np.isfinite(M).all(axis=2).tolist()
    assert _hex(C0) == _hex(M)
    counts = set()
    for y in range(h):
        for x in range(w):
            if valid[y, x]:
                want, cnt = _exact_v0(M, valid, y, x, R)
                counts.add(cnt)
                assert float(V0[y, x]).hex() == float(want).hex(), (name, R, y, x)
                assert V0[y, x] >= 0.0 and not np.signbit(V0[y, x])
            else:
                assert V0[y, x] == -1.0
    if name == "2x1 lone":
        assert counts == {1} and V0[0, 0].view(np.uint64) == 0       # a lone valid pixel: +0.0 exactly
    if name == "2x1 pair":
        assert counts == {2} and (V0 > 0.0).all()
    if name == "3x3 holes":
        assert valid.sum() == 7 and max(counts) == 7 and (R > 1) == (counts == {7})   # R = 1: the corners see fewer members
    # guided
    Cg, Vg, valid_g, a, d = sdh.prepare_albedo_spatial(M, A, floor, R)
    assert valid_g.tolist() == (np.isfinite(M).all(axis=2) & np.isfinite(A).all(axis=2)).tolist()
    assert _hex(a) == _hex(A)
    I = np.array(M)
    for y in range(h):
        for x in range(w):
            if valid_g[y, x]:
                dd = [_max(float(A[y, x, c]), floor) for c in range(3)]
                assert _hex(d[y, x]) == [float(t).hex() for t in dd]
                I[y, x] = [_r(Fraction(float(M[y, x, c])) / Fraction(dd[c])) for c in range(3)]
    assert _hex(Cg) == _hex(I)
    for y in range(h):
        for x in range(w):
            if valid_g[y, x]:
                want, _ = _exact_v0(I, valid_g, y, x, R)
                assert float(Vg[y, x]).hex() == float(want).hex(), (name, R, y, x)
            else:
                assert Vg[y, x] == -1.0 and _hex(Cg[y, x]) == _hex(M[y, x])
    if name.startswith("4x2"):
        assert not valid_g.all() and (d[valid_g] == floor).any() and (d[valid_g] > 1.0).any(), "the frame misses the floor"


def test_v0_is_never_negative_and_exactly_plus_zero_on_a_constant_window():
    """V0 >= 0 always.  On a window whose members all equal c, V0 = +0.0 exactly where the definition can give it: mu = s1 / cnt is c
    only if the in-order sums 2c .. cnt * c are exact, which the number format grants for any c of at most 47 significant bits (cnt <=
    49 < 2^6).  For other constants the definition itself — and so the device, which is held to it bit for bit — leaves a rounding
    residue: 0.1 in a 3 x 3 window gives mu = 0.1 + 1 ulp and V0 = 2.311e-34, not 0.  Those are held to the bound that follows from
    one rounding per addition, 2 * (cnt * 2^-52 * |c|)^2, instead."""
    rng = np.random.default_rng(13)
    for scale in (1e-300, 1e-3, 1.0, 1e6, 1e150):
        M = rng.standard_normal((9, 11, 3)) * scale
        M[4, 5, 1] = np.nan
        for R in (1, 2, 3):
            _, V0, valid = sdh.prepare_spatial(M, R)
            assert (V0[valid] >= 0.0).all() and not np.signbit(V0[valid]).any() and not np.isnan(V0[valid]).any()
            assert (V0[~valid] == -1.0).all()

    def few_bits(x):   # x cut to 47 significant bits
        m, e = np.frexp(x)
        return float(np.ldexp(np.trunc(m * 2.0 ** 47) / 2.0 ** 47, e))

    exact = [0.0, -0.0, 0.25, 0.75, 1.0, -7.25, few_bits(1e150), few_bits(1e-300), few_bits(0.1), few_bits(1.0 / 3.0), few_bits(-np.pi)]
    for value in exact:
        M = np.full((6, 7, 3), value)
        M[:, :, 1] = value * 2.0
        M[2, 3, 0] = np.inf                                 # a hole does not disturb a constant window
        for R in (1, 2, 3):
            _, V0, valid = sdh.prepare_spatial(M, R)
            assert (V0[valid].view(np.uint64) == 0).all(), (value, R)   # +0.0: not -0.0, not a rounding residue
            _, Vg, valid_g, _, _ = sdh.prepare_albedo_spatial(M, np.full_like(M, 0.5), 1e-3, R)
            assert (Vg[valid_g].view(np.uint64) == 0).all(), (value, R)
    residue = 0.0
    for value in (0.1, 1.0 / 3.0, np.pi, 1e-300 / 3.0, 1e150 / 7.0, -2.0 / 3.0):
        M = np.full((6, 7, 3), value)
        for R in (1, 2, 3):
            _, V0, valid = sdh.prepare_spatial(M, R)
            cnt = float((2 * R + 1) ** 2)
            assert valid.all() and (V0 >= 0.0).all() and not np.signbit(V0).any()
            assert (V0 <= 2.0 * (cnt * 2.0 ** -52 * abs(value)) ** 2).all(), (value, R, float(V0.max()))
            residue = max(residue, float((np.sqrt(V0) / abs(value)).max()))
    print(f"largest sqrt(V0) / |c| on a constant window of more than 47 significant bits: {residue:.3e}")
    assert residue > 0.0, "every constant gave +0.0: the docstring's example is out of date"
    # a window that is constant only in part: V0 = +0.0 where the whole window is, > 0 where it meets the step
    M = np.zeros((5, 12, 3)); M[:, 6:, :] = 0.75
    _, V0, _ = sdh.prepare_spatial(M, 1)
    assert (V0[:, :5] == 0.0).all() and (V0[:, 7:] == 0.0).all() and (V0[:, 5:7] > 0.0).all()


def test_the_threshold_chooses_the_route_and_albedo_one_is_the_plain_filter():
    rng = np.random.default_rng(17)
    M, M2 = rng.random((5, 7, 3)), rng.random((5, 7, 3)) * 0.2
    M[1, 2, 0] = np.nan
    A = rng.random((5, 7, 3))
    ldh = sdh.ldh
    for n in (1, 2, 3):
        for below in (1, 2, 3, 4):
            got = sdh.denoise_mean_spatial(M, M2, n, spatial_below=below, iterations=2)
            got_g = sdh.denoise_albedo_mean_spatial(M, M2, n, A, spatial_below=below, iterations=2)
            if n >= below:
                assert _hex(got) == _hex(ldh.denoise_mean(M, M2, n, iterations=2)), (n, below)
                assert _hex(got_g) == _hex(ldh.denoise_albedo_mean(M, M2, n, A, iterations=2)), (n, below)
            else:
                assert _hex(got) == _hex(sdh.denoise_mean_spatial(M, None, n, spatial_below=below, iterations=2))   # M2 is not looked at
                assert _hex(got) != _hex(ldh.denoise_mean(M, M2, n, iterations=2)), (n, below)
    assert _hex(sdh.denoise_mean_spatial(M, M2, 1, spatial_below=1)) == _hex(M)      # spatial_below = 1 never takes the spatial route
    assert _hex(sdh.denoise_mean_spatial(M, None, 1)) != _hex(M)                    # the default does, at one sample
    invalid = ~np.isfinite(M).all(axis=2)
    assert _hex(sdh.denoise_mean_spatial(M, None, 1)[invalid]) == _hex(M[invalid])  # a pixel that is not valid comes out unchanged
    ones = np.ones_like(M)
    for R in (1, 2, 3):
        assert _hex(sdh.denoise_albedo_mean_spatial(M, None, 1, ones, window_radius=R)) == _hex(sdh.denoise_mean_spatial(M, None, 1, window_radius=R))


# ---- refusals ----
def _filter(rt, guided, *, w=6, h=4, m=True, q=True, a=True, samples=1, spatial=None, params=None, out=True, rgba=True, ws=True, alias=None,
            misalign=False, ws_misalign=False):
    """One call of the spatial entry points on HOST buffers: only argument checks can answer (the first thing past them asks the HIP
    runtime which device owns d_mean_out, and host memory has none)."""
    lib = rt.amd_lib()
    n = min(w * h, 4096) if w > 0 and h > 0 else 1
    M, Q, A, O = ((C.c_double * (3 * n))() for _ in range(4))
    B = (C.c_uint8 * (4 * n + 4))()
    W = (C.c_uint8 * (96 * n + 32))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    out_ptr = C.addressof(O)
    if alias == "mean":
        out_ptr = C.addressof(M) + 8 * (3 * n - 1)
    elif alias == "m2":
        out_ptr = C.addressof(Q)
    elif alias == "albedo":
        out_ptr = C.addressof(A) - 8 * (3 * n - 1)
    head = [w, h, C.addressof(M) if m else None, C.addressof(Q) if q else None, samples]
    tail = [C.byref(spatial) if spatial is not None else None, C.byref(params) if params is not None else None, out_ptr if out else None,
            (C.addressof(B) + (1 if misalign else 0)) if rgba else None, ws_ptr if ws else None, None]
    if guided:
        rc = lib.rt_denoise_albedo_mean_spatial_device(*head, C.addressof(A) if a else None, *tail)
    else:
        rc = lib.rt_denoise_mean_spatial_device(*head, *tail)
    return rc, lib.rt_last_error().decode()


@pytest.mark.parametrize("guided", [False, True])
def test_every_invalid_argument_is_named_without_a_device(rt, guided):
    P = rt.DenoiseAlbedoParams if guided else rt.DenoiseParams
    S = rt.DenoiseSpatialParams
    make = rt.denoise_albedo_params if guided else rt.denoise_params
    sp = rt.denoise_spatial_params
    who = "rt_denoise_albedo_mean_spatial_device: " if guided else "rt_denoise_mean_spatial_device: "
    filter_struct = "rt_denoise_albedo_params" if guided else "rt_denoise_params"
    nan, inf = float("nan"), float("inf")
    cases = [
        # everything the means forms refuse
        (dict(m=False), "d_mean is null"),
        (dict(out=False), "d_mean_out is null"),
        (dict(ws=False), "d_workspace is null"),
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(samples=0), "samples"), (dict(samples=-4), "samples"),
        (dict(params=P(struct_size=12, iterations=4, sigma=4.0, eps=1e-6)), filter_struct + ".struct_size"),
        (dict(params=P(struct_size=48, iterations=4, sigma=4.0, eps=1e-6)), filter_struct + ".struct_size"),
        (dict(params=make(iterations=0)), "iterations"), (dict(params=make(iterations=7)), "iterations"),
        (dict(params=make(sigma=0.0)), "sigma"), (dict(params=make(sigma=nan)), "sigma"), (dict(params=make(sigma=inf)), "sigma"),
        (dict(params=make(eps=0.0)), "eps"), (dict(params=make(eps=nan)), "eps"),
        (dict(alias="mean"), "d_mean_out must not overlap"), (dict(alias="m2"), "d_mean_out must not overlap"),
        (dict(misalign=True), "d_rgba8"),
        (dict(ws_misalign=True), "d_workspace"),
        # the new ones
        (dict(spatial=S(struct_size=0, spatial_below=2, window_radius=1)), "rt_denoise_spatial_params.struct_size"),
        (dict(spatial=S(struct_size=4, spatial_below=2, window_radius=1)), "rt_denoise_spatial_params.struct_size"),
        (dict(spatial=S(struct_size=16, spatial_below=2, window_radius=1)), "rt_denoise_spatial_params.struct_size"),
        (dict(spatial=S(struct_size=10, spatial_below=2, window_radius=1)), "rt_denoise_spatial_params.struct_size"),
        (dict(spatial=sp(spatial_below=0)), "spatial_below"), (dict(spatial=sp(spatial_below=-3)), "spatial_below"),
        (dict(spatial=sp(window_radius=0)), "window_radius"), (dict(spatial=sp(window_radius=4)), "window_radius"),
        (dict(spatial=sp(window_radius=-1)), "window_radius"),
        (dict(q=False, samples=2), "d_m2 is null"),                                  # at the default threshold
        (dict(q=False, samples=1, spatial=sp(spatial_below=1)), "d_m2 is null"),     # spatial_below = 1: never the spatial route
        (dict(q=False, samples=5, spatial=sp(spatial_below=5)), "d_m2 is null"),
        # the documented order: pointers, the sample count, the spatial params in field order, d_m2, then the filter's params
        (dict(m=False, samples=0), "d_mean is null"),
        (dict(samples=0, spatial=sp(spatial_below=0)), "samples"),
        (dict(spatial=S(struct_size=4, spatial_below=0, window_radius=9)), "rt_denoise_spatial_params.struct_size"),
        (dict(spatial=sp(spatial_below=0, window_radius=9)), "spatial_below"),
        (dict(q=False, samples=2, spatial=sp(window_radius=9)), "window_radius"),
        (dict(q=False, samples=2, params=make(iterations=0)), "d_m2 is null"),
        (dict(spatial=sp(window_radius=9), params=make(iterations=0)), "window_radius"),
    ]
    if guided:
        cases += [
            (dict(a=False), "d_albedo_mean is null"),
            (dict(alias="albedo"), "d_mean_out must not overlap"),
            (dict(params=make(sigma_albedo=0.0)), "sigma_albedo"), (dict(params=make(albedo_floor=inf)), "albedo_floor"),
        ]
    for kw, field in cases:
        rc, msg = _filter(rt, guided, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith(who), (kw, msg)
        assert "d_sum" not in msg and "d_albedo_sum" not in msg, (kw, msg)
    # what is fine gets past every check: what answers then is the look-up of the device that owns a HOST pointer.  A null d_m2 is
    # fine below the threshold; a shorter struct of an older caller keeps the defaults it never knew
    fine = [dict(), dict(q=False), dict(rgba=False), dict(samples=2), dict(samples=7), dict(q=False, samples=4, spatial=sp(spatial_below=5)),
            dict(spatial=sp(window_radius=3)), dict(spatial=sp(spatial_below=1)), dict(q=False, spatial=S(struct_size=8, spatial_below=2, window_radius=99)),
            dict(q=False, params=make(iterations=6))]
    for kw in fine:
        rc, msg = _filter(rt, guided, **kw)
        assert rc != 0 and "not a device pointer" in msg and msg.startswith(who), (kw, rc, msg)
    # the means forms themselves still refuse a null d_m2 at any count
    lib = rt.amd_lib()
    n = 24
    M, O = (C.c_double * (3 * n))(), (C.c_double * (3 * n))()
    W = (C.c_uint8 * (96 * n + 32))()
    assert lib.rt_denoise_mean_device(6, 4, C.addressof(M), None, 1, None, C.addressof(O), None, (C.addressof(W) + 15) // 16 * 16, None) == -1
    assert "d_m2 is null" in lib.rt_last_error().decode()


def test_the_python_wrappers_check_their_frames(rt):
    with pytest.raises(rt.RtError, match="one shape"):
        rt.denoise_mean_spatial(np.zeros((4, 6, 3)), np.zeros((4, 5, 3)), 1)
    with pytest.raises(rt.RtError, match="one shape"):
        rt.denoise_albedo_mean_spatial(np.zeros((4, 6, 3)), None, 1, np.zeros((4, 6)))
    with pytest.raises(rt.RtError, match="albedo_mean"):
        rt.denoise_albedo_mean_spatial(np.zeros((4, 6, 3)), None, 1, None)
    with pytest.raises(TypeError):
        rt.denoise_mean_spatial(np.zeros((4, 6, 3)), None, 1, sigma_albedo=0.3)


def test_rtrace_refuses_the_spatial_flags_without_their_flags(rt, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "-o", str(tmp_path / "x")]
    cases = [
        (["--live", "--live-denoise-spatial"], "--live-denoise"), (["--live", "--live-denoise-spatial", "3"], "--live-denoise"),
        (["--live-denoise-spatial"], "--live-denoise"),
        (["--live", "--live-denoise", "--denoise-spatial-radius", "2"], "--live-denoise-spatial"),
        (["--live", "--denoise-spatial-radius", "2"], "--live-denoise-spatial"),
        # every existing refusal stands
        (["--live-denoise", "--live-denoise-spatial"], "--live"), (["--live-denoise-albedo", "--live-denoise-spatial", "2"], "--live"),
        (["--live", "--live-denoise", "--live-denoise-spatial", "--denoise"], "--denoise"),
        (["--live", "--live-denoise", "--live-denoise-spatial", "--gpus", "2"], "--live"),
        (["--live", "--live-denoise", "--live-denoise-spatial", "--denoise-albedo-sigma", "0.3"], "--live-denoise-albedo"),
    ]
    for extra, word in cases:
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (extra, r.stderr)
    for extra in (["--live", "--live-denoise", "--live-denoise-spatial", "0"],
                  ["--live", "--live-denoise", "--live-denoise-spatial", "--denoise-spatial-radius", "0"],
                  ["--live", "--live-denoise", "--live-denoise-spatial", "--denoise-spatial-radius", "4"]):
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "spatial" in r.stderr, (extra, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())
    usage = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--live-denoise-spatial" in usage and "--denoise-spatial-radius" in usage
