"""The film stage's C ABI without a GPU: the symbols and their Rust declarations, rt_film_bytes, and every invalid argument of
rt_film_device in the header's order (checked before any device work, the field named), which its host mirror rth_film refuses with
the same words."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

import film_helpers as fh

ROOT = Path(__file__).resolve().parent.parent


def test_the_symbols_are_exported_declared_and_bound(rt):
    lib = rt.amd_lib()
    header = (ROOT / "include" / "rt_amd.h").read_text()
    host_header = (ROOT / "include" / "rt_host.h").read_text()
    text = (ROOT / "INTEGRATION.md").read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_amd.so")], check=True, capture_output=True, text=True).stdout
    for fn in ("rt_film_bytes", "rt_film_device"):
        assert getattr(lib, fn) is not None and fn in rt.RT_AMD_SYMBOLS, fn
        assert re.search(r"\b(int|int64_t) " + fn + r"\(", header), fn
        assert f"pub fn {fn}(" in text, fn
        assert re.search(r" T " + fn + r"$", exported, flags=re.M), fn
    assert "film output (opt-in; nothing above changes)" in header
    for fn in ("rth_film", "rth_write_hdr", "rth_write_pfm", "rth_write_png16"):
        assert fn in rt.RT_HOST_SYMBOLS and re.search(r"\bint " + fn + r"\(", host_header), fn
        assert getattr(rt.host_lib(), fn) is not None
    for name in ("film_bytes", "film_device", "film_host", "film", "write_hdr", "write_pfm", "write_png16"):
        assert callable(getattr(rt, name)), name
    assert (rt.RT_FILM_RGBE, rt.RT_FILM_F32, rt.RT_FILM_RGB16) == (0, 1, 2) == fh.FORMATS
    for name, value in (("RGBE", 0), ("F32", 1), ("RGB16", 2)):
        assert re.search(rf"#define RT_FILM_{name} {value}\b", header)


def test_film_bytes(rt):
    lib = rt.amd_lib()
    for w, h in ((1, 1), (7, 3), (1200, 800), (257, 255), ((1 << 27) - 1, 1)):
        assert [lib.rt_film_bytes(w, h, f) for f in fh.FORMATS] == [w * h * 4, w * h * 12, w * h * 6]
        assert rt.film_bytes(w, h, "rgbe") == w * h * 4 and rt.film_bytes(w, h, "f32") == w * h * 12 and rt.film_bytes(w, h, "rgb16") == w * h * 6
    for w, h, f in ((0, 4, 0), (4, 0, 1), (-1, 4, 2), (1 << 14, 1 << 13, 0), (1 << 27, 1, 1), (4, 4, 3), (4, 4, -1)):
        assert lib.rt_film_bytes(w, h, f) == -1
        with pytest.raises(rt.RtError):
            rt.film_bytes(w, h, f)
    with pytest.raises(rt.RtError):
        rt.film_bytes(4, 4, "exr")


def _both(rt, *, w=6, h=4, v=True, out=True, spp=8, fmt=0, params=None, ws=True, ws_misalign=False, misalign=0, alias=False):
    """One call of rt_film_device on HOST buffers — only argument checks can answer: the first thing past them asks the HIP runtime which
    device owns the output — and, for the arguments the mirror has, the same call of rth_film: (rc, message, host rc, host message)"""
    lib, host = rt.amd_lib(), rt.host_lib()
    n = w * h if w > 0 and h > 0 else 1
    V = (C.c_double * (3 * n))()
    O = (C.c_uint8 * (12 * n + 8))()
    W = (C.c_uint8 * (64 * n + 64))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    out_ptr = (C.addressof(O) + 3) // 4 * 4 + misalign
    if alias:
        out_ptr = C.addressof(V) + 8 * (3 * n - 1) + misalign   # the last double of the values
    p = C.byref(params) if params is not None else None
    rc = lib.rt_film_device(w, h, C.addressof(V) if v else None, spp, None, p, fmt, out_ptr if out else None, ws_ptr if ws else None, None)
    msg = lib.rt_last_error().decode()
    if alias:
        return rc, msg, None, ""   # (the mirror would write there)
    hrc = host.rth_film(w, h, C.addressof(V) if v else None, spp, None, p, fmt, out_ptr if out else None)
    return rc, msg, hrc, host.rth_last_error().decode() if hrc else ""


def test_every_invalid_argument_is_named_without_a_device_and_the_mirror_says_the_same(rt):
    P = rt.TonemapParams
    nan, inf = float("nan"), float("inf")
    auto = rt.tonemap_params(auto_key=0.18)
    shared = [   # what both calls have
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(v=False), "values is null"),
        (dict(out=False), "out is null"),
        (dict(spp=0), "spp"), (dict(spp=-4), "spp"),
        (dict(fmt=3), "format"), (dict(fmt=-1), "format"),
        (dict(params=P(struct_size=12)), "struct_size"), (dict(params=P(struct_size=48)), "struct_size"),
        (dict(params=rt.tonemap_params(op=3)), "op"),
        (dict(params=rt.tonemap_params(exposure=0.0)), "exposure"), (dict(params=rt.tonemap_params(exposure=nan)), "exposure"),
        (dict(params=rt.tonemap_params(delta=0.0)), "delta"), (dict(params=rt.tonemap_params(delta=inf)), "delta"),
        (dict(params=rt.tonemap_params(auto_key=-0.18)), "auto_key"), (dict(params=rt.tonemap_params(auto_key=nan)), "auto_key"),
        (dict(params=rt.tonemap_params(white=0.0)), "white"), (dict(params=rt.tonemap_params(white=nan)), "white"),
    ]
    for kw, field in shared:
        rc, msg, hrc, hmsg = _both(rt, **kw)
        assert rc == -1 and hrc == -1, (kw, rc, hrc)
        assert field in msg and msg.startswith("rt_film_device: "), (kw, msg)
        assert hmsg.startswith("rth_film: "), (kw, hmsg)
        # the same words: the device call names its pointers d_values and d_out, the mirror values and out
        assert hmsg[len("rth_film: "):] == msg[len("rt_film_device: "):].replace("d_values", "values").replace("d_out", "out"), (kw, msg, hmsg)
    device_only = [   # the workspace, the stores' alignment and the overlap: the mirror has no workspace and writes bytes
        (dict(params=auto, ws=False), "d_workspace"), (dict(params=auto, ws_misalign=True), "d_workspace"),
        (dict(misalign=1), "4-byte"), (dict(misalign=2), "4-byte"), (dict(misalign=2, fmt=1), "4-byte"), (dict(misalign=1, fmt=2), "2-byte"),
        (dict(alias=True), "overlap"), (dict(alias=True, fmt=2), "overlap"),
    ]
    for kw, field in device_only:
        rc, msg, hrc, _ = _both(rt, **kw)
        assert rc == -1 and field in msg and msg.startswith("rt_film_device: "), (kw, rc, msg)
        assert hrc in (0, None), kw
    # the header's order: of two bad arguments the earlier one is named
    order = [dict(w=0), dict(v=False), dict(out=False), dict(spp=0), dict(fmt=7), dict(params=rt.tonemap_params(op=9, auto_key=0.18)),
             dict(params=auto, ws=False), dict(misalign=1), dict(alias=True)]
    names = ["width", "d_values", "d_out is null", "spp", "format", "op", "d_workspace", "aligned", "overlap"]
    for i in range(len(order) - 1):
        for j in range(i + 1, len(order)):
            if set(order[i]) & set(order[j]):
                continue   # (both need `params`: one struct cannot carry the two)
            msg = _both(rt, **order[i], **order[j])[1]
            assert names[i] in msg, (order[i], order[j], msg)
    # of the params, the op before the workspace it would need
    assert "op" in _both(rt, params=rt.tonemap_params(op=9, auto_key=0.18), ws=False)[1]
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(fmt=1), dict(fmt=2, misalign=2), dict(ws=False, ws_misalign=True), dict(params=auto, spp=1),
               dict(params=P(struct_size=8, op=2))):
        rc, msg, hrc, _ = _both(rt, **kw)
        assert rc != 0 and "not a device pointer" in msg, (kw, rc, msg)
        assert hrc == 0, kw


def test_the_python_wrappers_refuse_what_the_library_refuses(rt):
    import numpy as np
    f = np.ones((4, 6, 3))
    with pytest.raises(rt.RtError, match="format"):
        rt.film_host(f, 1, 5)
    with pytest.raises(rt.RtError, match="spp"):
        rt.film_host(f, 0, "f32")
    with pytest.raises(rt.RtError, match="no format"):
        rt.film_host(f, 1, "half")
    with pytest.raises(rt.RtError):
        rt.film_host(np.ones((4, 6)), 1, "f32")
    with pytest.raises(rt.RtError, match="shape"):
        rt.write_hdr("/nonexistent-dir/x.hdr", np.zeros((4, 6, 3), dtype=np.uint8))
    with pytest.raises(rt.RtError, match="cannot write"):
        rt.write_pfm("/nonexistent-dir/x.pfm", np.zeros((4, 6, 3), dtype=np.float32))
