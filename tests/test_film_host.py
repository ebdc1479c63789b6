"""The film stage's host mirror (rth_film) and the three file writers on the CPU, against the numpy restatement of include/rt_amd.h
"film output" (tests/film_helpers.py), bit for bit: every format under every operator in the sums, map and means forms; RGBE's exact
bracket; the 16-bit frame's high bytes against the tone-mapping stage's; the f32 frame against the means; and the files read back by the
readers written in the helpers."""
from fractions import Fraction

import numpy as np
import pytest

import film_helpers as fh
import tonemap_helpers as th

# clamp, Reinhard with white = +inf and 4, ACES
CURVES = [(th.CLAMP, th.INF), (th.REINHARD, th.INF), (th.REINHARD, 4.0), (th.ACES, th.INF)]
CURVE_IDS = ["clamp", "reinhard", "reinhard-white4", "aces"]


@pytest.fixture(scope="module")
def frames():
    out = {("values",) + s: th.value_frame(*s, shift=s[0]) for s in th.SIZES}
    out.update({("radiance",) + s: th.radiance_frame(*s, seed=sum(s)) for s in th.SIZES})
    out[("edges",)] = fh.edge_frame()
    for f in out.values():
        f.setflags(write=False)
    return out


def _same(fmt, got, want):
    return np.array_equal(fh.as_bits(fmt, got), want)


def test_the_restated_logarithm_is_the_oracles_and_the_restated_gamma_gives_the_pinned_bytes(rt):
    import oracle_lib
    orc_log = oracle_lib.lib().orc_log
    rng = np.random.default_rng(7)
    xs = np.concatenate([10.0 ** rng.uniform(-300, 300, 400), [5e-324, 2.0 ** -1030, 1.0, 2.0, 0.5, np.sqrt(0.5), np.sqrt(2.0), 1e308, 0.18]])
    assert [float(v).hex() for v in fh.np_log(xs)] == [orc_log(float(x)).hex() for x in xs]
    y = np.concatenate([10.0 ** rng.uniform(-12, 1, 3000), fh.edge_pixels().ravel()])
    y = y[:len(y) // 3 * 3].reshape(1, -1, 3)
    assert np.array_equal(fh.rgb16_of(y) >> 8, rt.resolve_rgb8_host(y.shape[1], 1, 1, y))


@pytest.mark.parametrize("fmt", fh.FORMATS, ids=lambda f: fh.FORMAT_NAMES[f])
@pytest.mark.parametrize("curve", CURVES, ids=CURVE_IDS)
def test_the_mirror_is_the_restatement_bit_for_bit(rt, frames, fmt, curve):
    op, white = curve
    for key, f in frames.items():
        kw = dict(op=op, exposure=1.7, white=white)
        assert _same(fmt, rt.film_host(f, 1, fmt, **kw), fh.expected(fmt, f, 1, op=op, scale=1.7, white=white)), key           # means
    for key in (("values", 257, 255), ("radiance", 16, 16), ("edges",)):
        f = frames[key]
        h, w = f.shape[:2]
        kw = dict(op=op, exposure=0.5, white=white)
        assert _same(fmt, rt.film_host(f, 3, fmt, **kw), fh.expected(fmt, f, 3, op=op, scale=0.5, white=white)), key           # sums
        spp_map = th.spp_map_for(w, h)
        assert _same(fmt, rt.film_host(f, 1, fmt, spp_map=spp_map, **kw), fh.expected(fmt, f, 1, spp_map, op=op, scale=0.5, white=white)), key


@pytest.mark.parametrize("fmt", fh.FORMATS, ids=lambda f: fh.FORMAT_NAMES[f])
def test_auto_exposure_is_the_fixed_exposure_at_the_log_averages_scale(rt, frames, fmt):
    for key in (("radiance", 257, 255), ("radiance", 1, 1), ("edges",)):
        f = frames[key]
        _, lavg, count, _ = rt.log_average_luminance_host(f, 1)
        scale = th.scale_of(1.5, 0.18, lavg, count)
        got = rt.film_host(f, 1, fmt, op="aces", exposure=1.5, auto_key=0.18)
        assert _same(fmt, got, fh.expected(fmt, f, 1, op=th.ACES, scale=scale)), key
        assert np.array_equal(fh.as_bits(fmt, got), fh.as_bits(fmt, rt.film_host(f, 1, fmt, op="aces", exposure=scale))), key


@pytest.mark.parametrize("curve", CURVES, ids=CURVE_IDS)
def test_rgbe_brackets_its_value_exactly(rt, frames, curve):
    op, white = curve
    seen = set()
    for key in (("edges",), ("radiance", 16, 16), ("values", 16, 16)):
        f = frames[key]
        y = fh.value(f, 1, op=op, scale=1.7, white=white)
        rgbe = rt.film_host(f, 1, "rgbe", op=op, exposure=1.7, white=white)
        c = fh.rgbe_channel(y)
        lo, hi = fh.rgbe_decode_bounds(rgbe)
        E = rgbe[..., 3].astype(int)
        v = c.max(axis=2)
        zero = v < Fraction(2) ** -128
        assert np.array_equal(zero, (rgbe == 0).all(axis=2)) and np.array_equal(zero, E == 0), key   # the zero pixel exactly where v < 2^-128
        live = ~zero
        assert (lo[live] <= c[live]).all() and (c[live] < hi[live]).all(), key
        assert (rgbe[..., :3].max(axis=2)[live] >= 128).all() and (E[live] >= 1).all(), key
        seen |= {bool(x) for x in zero.ravel()}
    assert seen == {True, False}


@pytest.mark.parametrize("curve", CURVES, ids=CURVE_IDS)
def test_the_16_bit_high_bytes_are_the_tone_mapping_stages(rt, frames, curve):
    op, white = curve
    for key, f in frames.items():
        kw = dict(op=op, exposure=1.7, white=white)
        assert np.array_equal(rt.film_host(f, 1, "rgb16", **kw) >> 8, rt.tonemap_host(f, 1, **kw)), key
    f = frames[("radiance", 257, 255)]
    spp_map = th.spp_map_for(257, 255)
    kw = dict(op=op, white=white, auto_key=0.18)
    assert np.array_equal(rt.film_host(f, 1, "rgb16", spp_map=spp_map, **kw) >> 8, rt.tonemap_host(f, 1, spp_map=spp_map, **kw))


def test_with_the_defaults_f32_is_the_means(rt, frames):
    for key, f in frames.items():
        got = rt.film_host(f, 1, "f32")
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), fh.f32_bits_of(f)), key
    f = frames[("radiance", 16, 16)]
    with np.errstate(all="ignore"):
        want = (f * (1.0 / 12)).astype(np.float32)
    assert np.array_equal(rt.film_host(f, 12, "f32"), want, equal_nan=True)
    rgbe = rt.film_host(f, 1, "rgbe")                      # and RGBE holds what lies above 1
    lo, _ = fh.rgbe_decode_bounds(rgbe)
    assert max(lo.ravel()) > 1


def _film_frame(fmt, w, h, kind):
    """a frame in `fmt` to write: `runs` has long constant stretches (and one longer than a run can be), `noise` has none"""
    rng = np.random.default_rng(w * 31 + h)
    dtype, ch = {fh.RGBE: (np.uint8, 4), fh.F32: (np.uint32, 3), fh.RGB16: (np.uint16, 3)}[fmt]
    if kind == "noise":
        a = rng.integers(0, np.iinfo(dtype).max, size=(h, w, ch), endpoint=True, dtype=dtype)
    else:
        a = np.zeros((h, w, ch), dtype=dtype)
        x = 0
        while x < w:
            n = int(rng.choice([1, 2, 3, 4, 5, 127, 128, 129, 300]))
            a[:, x:x + n] = rng.integers(0, np.iinfo(dtype).max, size=(h, 1, ch), endpoint=True, dtype=dtype)
            x += n
    return a


SHAPES = [(1, 1, "noise"), (7, 3, "noise"), (8, 1, "noise"), (8, 1, "runs"), (32767, 1, "runs"), (32768, 1, "runs"), (700, 5, "runs"), (61, 9, "noise")]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def test_the_files_read_back_as_the_arrays_written(rt, tmp_path, shape):
    w, h, kind = shape
    rgbe = _film_frame(fh.RGBE, w, h, kind)
    rt.write_hdr(tmp_path / "a.hdr", rgbe)
    back, rle = fh.read_hdr(tmp_path / "a.hdr")
    assert np.array_equal(back, rgbe) and rle == (8 <= w <= 32767)
    assert (tmp_path / "a.hdr").read_bytes().startswith(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
    if kind == "runs" and w >= 700:
        assert ((tmp_path / "a.hdr").stat().st_size < rgbe.size // 2) == rle, "constant stretches must go out as runs where the code exists"

    bits = _film_frame(fh.F32, w, h, kind)
    rt.write_pfm(tmp_path / "a.pfm", bits.view(np.float32))
    assert np.array_equal(fh.read_pfm(tmp_path / "a.pfm"), bits)
    assert (tmp_path / "a.pfm").read_bytes().startswith(b"PF\n%d %d\n-1.0\n" % (w, h))

    rgb16 = _film_frame(fh.RGB16, w, h, kind)
    rt.write_png16(tmp_path / "a.png", rgb16)
    back, filters = fh.read_png16(tmp_path / "a.png")
    assert np.array_equal(back, rgb16) and len(filters) == h


def test_the_16_bit_png_uses_the_adaptive_filters_and_pillow_opens_it(rt, tmp_path):
    j, i = np.mgrid[0:40, 0:64]
    smooth = np.stack([i * 1000 + j * 3, j * 1500 + i, (i + j) * 600], axis=2).astype(np.uint16)   # gradients: the filters have work to do
    rt.write_png16(tmp_path / "g.png", smooth)
    back, filters = fh.read_png16(tmp_path / "g.png")
    assert np.array_equal(back, smooth) and set(filters) - {0}, filters
    try:
        from PIL import Image
    except ImportError:
        return                                             # (only this assertion needs Pillow)
    with Image.open(tmp_path / "g.png") as im:
        assert im.size == (64, 40) and im.mode in ("RGB;16", "RGB", "I;16") and im.format == "PNG"


def test_the_8_bit_png_is_still_the_bytes_it_was(rt, tmp_path):
    """the writer's filter routine now serves two pixel strides: the 8-bit file of a fixed frame is pinned by its own reader and by size"""
    rgb = rt.film_host(th.radiance_frame(61, 9, seed=3), 1, "rgbe")[..., :3].copy()
    rt.write_png(tmp_path / "p.png", rgb)
    hs = rt.host_lib()
    import ctypes as C
    w, h = C.c_int32(), C.c_int32()
    out = np.zeros(61 * 9 * 3, dtype=np.uint8)
    assert hs.rth_load_image(str(tmp_path / "p.png").encode(), C.byref(w), C.byref(h), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size) == 0
    assert (w.value, h.value) == (61, 9) and np.array_equal(out.reshape(9, 61, 3), rgb)
