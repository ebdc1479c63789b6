"""Panoramas' C ABI without a GPU: the symbols and their Rust declarations, and every invalid argument of rt_camera_cube_faces and
rt_panorama_device in the header's order (checked before any device work, the field named); rth_panorama refuses the same things with the
same words."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_camera_cube_faces", "rt_panorama_tables", "rt_panorama_device")


def test_the_symbols_are_exported_declared_and_bound(rt):
    lib = rt.amd_lib()
    header = (ROOT / "include" / "rt_amd.h").read_text()
    text = (ROOT / "INTEGRATION.md").read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_amd.so")], check=True, capture_output=True, text=True).stdout
    for fn in SYMBOLS + ("rt_device_upload",):
        assert getattr(lib, fn) is not None
        assert fn in rt.RT_AMD_SYMBOLS, fn
        assert re.search(r"\bint " + fn + r"\(", header), fn
        assert f"pub fn {fn}(" in text, fn
        assert re.search(r" T " + fn + r"$", exported, flags=re.M), fn
    assert "panoramas (opt-in; nothing above changes)" in header
    host_header = (ROOT / "include" / "rt_host.h").read_text()
    host_exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_host.so")], check=True, capture_output=True, text=True).stdout
    assert "rth_panorama" in rt.RT_HOST_SYMBOLS and re.search(r"\bint rth_panorama\(", host_header) and re.search(r" T rth_panorama$", host_exported, flags=re.M)
    for name in ("cube_face_cameras", "panorama_tables", "panorama_device", "panorama_host", "panorama"):
        assert callable(getattr(rt, name)), name
    assert callable(rt.DeviceScene.render_panorama)
    makefile = (ROOT / "rust-tracing_amd" / "csrc" / "Makefile").read_text()
    assert makefile.count("rt_panorama.o") >= 3 and "rt_panorama_shared.h" in makefile and "-c -o /dev/null rt_panorama.hip" in makefile


def test_cube_faces_refuses_in_the_headers_order(rt):
    lib = rt.amd_lib()
    like, out = rt.Camera(), (rt.Camera * 6)()

    def call(like_=True, out_=True, F=8, g=1):
        rc = lib.rt_camera_cube_faces(C.byref(like) if like_ else None, None, F, g, out if out_ else None)
        return rc, lib.rt_last_error().decode()
    assert call()[0] == 0 and call(F=2, g=0)[0] == 0 and call(F=16384, g=8191)[0] == 0 and call(F=3, g=1)[0] == 0
    order = [(dict(like_=False), "like is null"), (dict(out_=False), "out is null"), (dict(F=1), "face_size must be from 2 to 16384"),
             (dict(g=-1), "guard must not be negative"), (dict(F=4, g=2), "face_size - 2 * guard must be at least 1")]
    for kw, words in order + [(dict(F=16385), "face_size must be"), (dict(F=0), "face_size must be"), (dict(F=9, g=5), "face_size - 2 * guard"),
                              (dict(F=16384, g=8192), "face_size - 2 * guard"), (dict(F=2, g=2 ** 31 - 1), "face_size - 2 * guard")]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("rt_camera_cube_faces: " + words), (kw, msg)
    # of two bad arguments the earlier one is named (F = 1 with g = 1 is bad as a face size and as F - 2 g)
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kw = {**order[b][0], **order[a][0]} if not (set(order[a][0]) & set(order[b][0])) else None
            if kw is None:
                continue
            rc, msg = call(**kw)
            assert rc == -1 and order[a][1] in msg, (kw, msg)
    rc, msg = call(F=1, g=1)
    assert rc == -1 and "face_size must be" in msg
    rc, msg = call(F=1, g=-1)
    assert rc == -1 and "face_size must be" in msg


def _device(rt, *, w=6, h=3, tables=True, faces=True, F=4, g=1, spp=2, out=True, alias=None):
    """One call of rt_panorama_device on HOST buffers: only argument checks can answer (the first thing past them asks the HIP runtime
    which device owns the output, and host memory has none)."""
    lib = rt.amd_lib()
    n = w * h if w > 0 and h > 0 and w * h < 1 << 20 else 1
    f = F if 2 <= F <= 64 else 2
    gap = 3 * n + 8   # one allocation, the three buffers far enough apart that an alias meets only the buffer it aims at
    n_t = (2 * (abs(w) + abs(h))) % (1 << 20) + 2
    B = (C.c_double * (n_t + 18 * f * f + 3 * n + 2 * gap))()
    T = C.addressof(B)
    S = T + 8 * (n_t + gap)
    O = S + 8 * (18 * f * f + gap)
    out_ptr = O
    if alias == "tables_last":
        out_ptr = T + 8 * (2 * w + 2 * h - 1)
    elif alias == "faces_last":
        out_ptr = S + 8 * (18 * f * f - 1)
    elif alias == "faces_first":
        out_ptr = S - 8 * (3 * n - 1)
    rc = lib.rt_panorama_device(w, h, T if tables else None, S if faces else None, F, g, spp, out_ptr if out else None, None)
    return rc, lib.rt_last_error().decode()


def test_every_invalid_argument_is_named_without_a_device_in_the_headers_order(rt):
    cases = [(dict(w=0), "width and height must be positive"), (dict(h=-3), "width and height must be positive"),
             (dict(w=1 << 14, h=1 << 13), "width x height must be below 2^27 pixels"),
             (dict(F=1), "face_size must be from 2 to 16384"), (dict(F=16385), "face_size must be from 2 to 16384"),
             (dict(g=-1), "guard must not be negative"), (dict(F=4, g=2), "face_size - 2 * guard must be at least 1"),
             (dict(tables=False), "d_tables is null"), (dict(faces=False), "d_faces is null"), (dict(out=False), "d_mean_out is null"),
             (dict(spp=0), "spp must be at least 1"), (dict(spp=-4), "spp must be at least 1"),
             (dict(alias="tables_last"), "d_mean_out must not overlap d_tables"), (dict(alias="faces_last"), "d_mean_out must not overlap d_faces"),
             (dict(alias="faces_first"), "d_mean_out must not overlap d_faces")]
    for kw, words in cases:
        rc, msg = _device(rt, **kw)
        assert rc == -1 and msg == "rt_panorama_device: " + words, (kw, rc, msg)
    order = [(dict(w=0), "width"), (dict(F=1), "face_size must be"), (dict(g=-1), "guard"), (dict(tables=False), "d_tables"), (dict(faces=False), "d_faces"),
             (dict(out=False), "d_mean_out is null"), (dict(spp=0), "spp"), (dict(alias="faces_last"), "overlap")]
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            if order[b][0].get("alias") and "out" in order[a][0]:
                continue   # (a null output cannot overlap anything)
            rc, msg = _device(rt, **{**order[b][0], **order[a][0]})
            assert rc == -1 and order[a][1] in msg, (order[a], order[b], msg)
    # what is fine gets past every check: what answers then is the look-up of the device that owns a HOST pointer
    for kw in (dict(), dict(F=2, g=0), dict(F=3, g=1), dict(spp=1), dict(w=1, h=1)):
        rc, msg = _device(rt, **kw)
        assert rc != 0 and "overlap" not in msg and "must" not in msg and "null" not in msg, (kw, rc, msg)


def test_the_host_mirror_refuses_the_same_things_with_the_same_words(rt):
    lib, host = rt.amd_lib(), rt.host_lib()
    T, S, O = (C.c_double * 18)(), (C.c_double * (18 * 16))(), (C.c_double * 54)()
    for kw in (dict(w=0), dict(h=0), dict(w=1 << 14, h=1 << 13), dict(F=1), dict(F=16385), dict(g=-1), dict(F=4, g=2), dict(tables=None), dict(faces=None),
               dict(out=None), dict(spp=0), dict(out=C.addressof(T) + 8 * 17), dict(out=C.addressof(S) + 8 * (18 * 16 - 1))):
        a = dict(w=6, h=3, tables=C.addressof(T), faces=C.addressof(S), F=4, g=1, spp=1, out=C.addressof(O))
        a.update(kw)
        assert lib.rt_panorama_device(a["w"], a["h"], a["tables"], a["faces"], a["F"], a["g"], a["spp"], a["out"], None) == -1, kw
        assert host.rth_panorama(a["w"], a["h"], a["tables"], a["faces"], a["F"], a["g"], a["spp"], a["out"]) == -1, kw
        dev, mirror = lib.rt_last_error().decode(), host.rth_last_error().decode()
        assert dev.startswith("rt_panorama_device: ") and mirror.startswith("rth_panorama: ")
        tail = dev[len("rt_panorama_device: "):]
        assert mirror[len("rth_panorama: "):] == tail.replace("d_mean_out", "out_mean").replace("d_tables", "tables").replace("d_faces", "faces"), (kw, dev, mirror)
    assert host.rth_panorama(6, 3, C.addressof(T), C.addressof(S), 4, 1, 1, C.addressof(O)) == 0


def test_the_tables_call_refuses_a_bad_size_and_a_null(rt):
    lib = rt.amd_lib()
    t = np.zeros(8)
    for args, words in (((0, 2, t.ctypes.data), "width and height"), ((2, -1, t.ctypes.data), "width and height"),
                        ((1 << 14, 1 << 13, t.ctypes.data), "2^27"), ((2, 2, None), "tables is null")):
        assert lib.rt_panorama_tables(*args) == -1 and words in lib.rt_last_error().decode(), args
    assert lib.rt_panorama_tables(2, 2, t.ctypes.data) == 0
