"""Shared by the film-output tests (not a test module): the normative definition of include/rt_amd.h "film output" in numpy, and
independent readers of the three files.  The value before encoding is tonemap_helpers' restatement of the stage.  RGBE is restated on
the integers of the doubles' bits — no multiplication, no frexp; F32 is numpy's own conversion with the NaNs made the one NaN; the 16-bit
quantiser runs on a numpy restatement of the fixed logarithm and exponential (DESIGN.md "Device math"), which test_film_host.py holds
against the oracle library's orc_log and against the pinned 8-bit output stage."""
import struct
import zlib

import numpy as np

import tonemap_helpers as th

RGBE, F32, RGB16 = 0, 1, 2
FORMATS = (RGBE, F32, RGB16)
FORMAT_NAMES = {RGBE: "rgbe", F32: "f32", RGB16: "rgb16"}
PIXEL_BYTES = {RGBE: 4, F32: 12, RGB16: 6}
TOP = 255.0 * 2.0 ** 119   # the largest value an RGBE pixel holds
INF, NAN = float("inf"), float("nan")


def _pred(x):
    return float(np.nextafter(np.float64(x), -INF))


def _succ(x):
    return float(np.nextafter(np.float64(x), INF))


def edge_pixels():
    """(n, 3) float64: every edge of the three encoders, alone in a pixel, as a pixel's largest channel beside smaller ones, and mixed"""
    singles = [0.0, -0.0, -1.0, -1e-300, -1e300, NAN, INF, -INF, 5e-324, 2.0 ** -1030, 2.0 ** -129, 2.0 ** -128, _pred(2.0 ** -128),
               _succ(2.0 ** -128), 1.0, 2.0, 0.5, 2.0 ** -127, 2.0 ** -126, 2.0 ** -149, 2.0 ** -150, _succ(2.0 ** -150), 1.5 * 2.0 ** -149,
               2.0 ** 100, 2.0 ** 126, _pred(1.0), _pred(2.0), _pred(256.0), _pred(2.0 ** -20), _pred(2.0 ** 120), TOP, _succ(TOP), _pred(TOP),
               2.0 ** 127, _pred(2.0 ** 128), 2.0 ** 128, 1e300, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50,
               0.18, 4.0, 15.0, 0.99999, 0.999, 0.9999999, 1.0 / 256, 1.0 / 65536]
    px = []
    for v in singles:
        px += [(v, v, v), (v, 0.0, 0.0), (0.0, v, 0.25), (0.3, 0.7, v)]
    for v in (1.0, 15.0, 2.0 ** -100, TOP, _pred(2.0), 2.0 ** 126 * 1.37, INF):   # other channels 2^-9 and 2^-60 of the largest, and around them
        small = v if v != INF else TOP
        px += [(v, small * 2.0 ** -9, small * 2.0 ** -60), (small * 2.0 ** -60, v, small * 2.0 ** -9), (small * 2.0 ** -8, _pred(small * 2.0 ** -8), v),
               (small * 2.0 ** -9 * 1.999, v, -small), (NAN, v, small * 0.5)]
    px += [(2.0 ** -128, 2.0 ** -129, 2.0 ** -130), (_pred(2.0 ** -128), _pred(2.0 ** -128), 0.0), (-INF, NAN, -0.0), (INF, INF, 1.0), (INF, -1.0, 2.0 ** 127)]
    return np.array(px, dtype=np.float64)


def edge_frame():
    px = edge_pixels()
    return px.reshape(1, len(px), 3)


# ---- the value before encoding -------------------------------------------------------------------------------------------------------------

def value(values, spp, spp_map=None, *, op=th.CLAMP, scale=1.0, white=th.INF):
    """y = rt_tonemap(op, m * scale, w2): (h, w, 3) float64"""
    m = th.means(values, spp, spp_map)
    with np.errstate(all="ignore"):
        x = m * np.float64(scale)
    return th.operator(op, x, white)


# ---- RT_FILM_RGBE on integers --------------------------------------------------------------------------------------------------------------

TOP_BITS = int(np.float64(TOP).view(np.uint64))


def rgbe_of(y):
    """(h, w, 3) float64 -> (h, w, 4) uint8.  A positive double's bits order as its value does, so clamping, the maximum and the
    threshold are integer comparisons; with field F and significand M (the implicit bit set), c = M * 2^(F - 1075) and e = Fv - 1022, so
    floor(c * 2^(8 - e)) = M >> (45 + Fv - F)."""
    b = np.ascontiguousarray(y, dtype=np.float64).view(np.uint64)
    positive = (b >> np.uint64(63) == 0) & (b != 0) & (b <= np.uint64(0x7FF0000000000000))   # y > 0, +inf included; NaN, zero, negatives: 0
    c = np.where(positive, np.minimum(b, np.uint64(TOP_BITS)), np.uint64(0))
    v = c.max(axis=2)
    live = v >= np.uint64((1023 - 128) << 52)
    fv = (v >> np.uint64(52)).astype(np.int64)
    f = (c >> np.uint64(52)).astype(np.int64)
    man = c & np.uint64((1 << 52) - 1)
    m_int = np.where(f > 0, man | np.uint64(1 << 52), man)      # a subnormal channel: no implicit bit, exponent as field 1
    shift = 45 + fv[..., None] - np.maximum(f, 1)                 # >= 45: a channel is at most v
    byte = np.where(shift < 64, m_int >> np.minimum(shift, 63).astype(np.uint64), np.uint64(0))
    assert byte.max(initial=0) < 256
    out = np.zeros(b.shape[:2] + (4,), dtype=np.uint8)
    out[..., :3] = byte
    out[..., 3] = fv - 1022 + 128
    out[~live] = 0
    return out


def rgbe_decode_bounds(rgbe):
    """(lo, hi) as exact python Fractions per value: b * 2^(E - 136) <= c < (b + 1) * 2^(E - 136); E == 0: both 0"""
    from fractions import Fraction
    rgbe = np.asarray(rgbe)
    lo = np.empty(rgbe.shape[:2] + (3,), dtype=object)
    hi = np.empty_like(lo)
    for idx in np.ndindex(rgbe.shape[:2]):
        E = int(rgbe[idx + (3,)])
        unit = Fraction(2) ** (E - 136) if E else Fraction(0)
        for k in range(3):
            lo[idx + (k,)] = int(rgbe[idx + (k,)]) * unit
            hi[idx + (k,)] = (int(rgbe[idx + (k,)]) + 1) * unit
    return lo, hi


def rgbe_channel(y):
    """c of the definition per value, as exact Fractions: y where y > 0, capped at 255 * 2^119; else 0"""
    from fractions import Fraction
    y = np.asarray(y, dtype=np.float64)
    out = np.empty(y.shape, dtype=object)
    for idx in np.ndindex(y.shape):
        v = float(y[idx])
        out[idx] = Fraction(min(v, TOP)) if v > 0.0 else Fraction(0)
    return out


# ---- RT_FILM_F32 -----------------------------------------------------------------------------------------------------------------------------

def f32_bits_of(y):
    """(h, w, 3) float64 -> (h, w, 3) uint32: numpy's round-to-nearest-even conversion, every NaN the one NaN"""
    with np.errstate(all="ignore"):
        f = np.asarray(y, dtype=np.float64).astype(np.float32)
    bits = f.view(np.uint32).copy()
    bits[np.isnan(f)] = 0x7FC00000
    return bits


# ---- RT_FILM_RGB16: the fixed ln and exp in numpy, then the quantiser -------------------------------------------------------------------------

def np_log(x):
    """rt_log for finite x > 0 (DESIGN.md "Device math"): every operation a numpy operation, rounded once"""
    x = np.asarray(x, dtype=np.float64).copy()
    b = x.view(np.uint64)
    e = (b >> np.uint64(52)).astype(np.int64)
    sub = e == 0
    x[sub] = x[sub] * 18014398509481984.0
    b = x.view(np.uint64)
    e = np.where(sub, (b >> np.uint64(52)).astype(np.int64) - 54, e)
    mant = b & np.uint64(0x000FFFFFFFFFFFFF)
    big = mant >= np.uint64(0x6A09E667F3BCD)
    m = np.where(big, (mant | np.uint64(0x3FE0000000000000)).view(np.float64), (mant | np.uint64(0x3FF0000000000000)).view(np.float64))
    dk = np.where(big, e - 1022, e - 1023).astype(np.float64)
    Lg = [6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01, 1.818357216161805012e-01,
          1.531383769920937332e-01, 1.479819860511658591e-01]
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (Lg[1] + w * (Lg[3] + w * Lg[5]))
    t2 = z * (Lg[0] + w * (Lg[2] + w * (Lg[4] + w * Lg[6])))
    R = t2 + t1
    hfsq = (0.5 * f) * f
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)


def np_exp(x):
    """rt_exp for |x| <= 700"""
    x = np.asarray(x, dtype=np.float64)
    ln2_hi, ln2_lo, inv_ln2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
    P = [1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05, -1.65339022054652515390e-06, 4.13813679705723846039e-08]
    ax = np.abs(x)
    reduced = ax > 0.34657359027997264
    tiny = ~reduced & (ax < 3.725290298461914e-09)
    t = np.where(reduced, np.trunc(inv_ln2 * x + np.where(x < 0.0, -0.5, 0.5)), 0.0)
    k = t.astype(np.int64)
    hi = np.where(reduced, x - t * ln2_hi, x)
    lo = np.where(reduced, t * ln2_lo, 0.0)
    xr = np.where(reduced, hi - lo, x)
    tt = xr * xr
    c = xr - tt * (P[0] + tt * (P[1] + tt * (P[2] + tt * (P[3] + tt * P[4]))))
    plain = 1.0 - ((xr * c) / (c - 2.0) - xr)
    y = 1.0 - ((lo - (xr * c) / (2.0 - c)) - hi)
    scaled = (y.view(np.uint64) + (k.astype(np.uint64) << np.uint64(52))).view(np.float64)   # (mod 2^64, as the product's addition)
    return np.where(tiny, 1.0 + x, np.where(k == 0, plain, scaled))


def gamma_of(y):
    """rt_gamma_encode: NaN stays, +-0 -> 0, negatives -> NaN, +inf stays, else exp(ln(y) * (1 / 2.2))"""
    y = np.asarray(y, dtype=np.float64)
    out = np.full(y.shape, NAN)
    out[y == 0.0] = 0.0
    out[y == INF] = INF
    ok = (y > 0.0) & (y < INF)
    with np.errstate(all="ignore"):
        out[ok] = np_exp(np_log(y[ok]) * (1.0 / 2.2))
    return out


def rgb16_of(y):
    """(h, w, 3) float64 -> (h, w, 3) uint16: (u16)(65536 * clamp(g, 0, 0.99999)), NaN -> 0"""
    g = gamma_of(y)
    with np.errstate(all="ignore"):
        c = np.where(g < 0.0, 0.0, np.where(g > 0.99999, 0.99999, g))
        q = np.floor(65536.0 * c)
    return np.where(np.isnan(g), 0.0, q).astype(np.uint16)


def expected(fmt, values, spp, spp_map=None, **kw):
    """the frame in `fmt` as film_host / film return it: (h, w, 4) uint8, (h, w, 3) uint32 (the floats' bits) or (h, w, 3) uint16"""
    y = value(values, spp, spp_map, **kw)
    return {RGBE: rgbe_of, F32: f32_bits_of, RGB16: rgb16_of}[fmt](y)


def as_bits(fmt, frame):
    """a frame from the library in the form `expected` gives: floats as their bits"""
    frame = np.asarray(frame)
    return frame.view(np.uint32) if fmt == F32 else frame


# ---- readers of the three files, written here ------------------------------------------------------------------------------------------------

def read_hdr(path):
    """(h, w, 4) uint8 and whether the scanlines were run-length coded"""
    data = open(path, "rb").read()
    head, _, body = data.partition(b"\n\n")
    lines = head.split(b"\n")
    assert lines[0] == b"#?RADIANCE" and b"FORMAT=32-bit_rle_rgbe" in lines[1:], head
    res, _, body = body.partition(b"\n")
    y_sign, h, x_sign, w = res.split()
    assert (y_sign, x_sign) == (b"-Y", b"+X"), res
    w, h = int(w), int(h)
    out = np.zeros((h, w, 4), dtype=np.uint8)
    at, rle = 0, False
    for j in range(h):
        if 8 <= w <= 32767 and body[at] == 2 and body[at + 1] == 2 and not body[at + 2] & 0x80:
            assert (body[at + 2] << 8 | body[at + 3]) == w
            at += 4
            rle = True
            for c in range(4):
                x = 0
                while x < w:
                    n = body[at]
                    if n > 128:
                        n -= 128
                        assert n >= 1 and x + n <= w
                        out[j, x:x + n, c] = body[at + 1]
                        at += 2
                    else:
                        assert 1 <= n and x + n <= w
                        out[j, x:x + n, c] = np.frombuffer(body, np.uint8, n, at + 1)
                        at += 1 + n
                    x += n
        else:
            out[j] = np.frombuffer(body, np.uint8, w * 4, at).reshape(w, 4)
            at += w * 4
    assert at == len(body), "bytes behind the last scanline"
    return out, rle


def read_pfm(path):
    """(h, w, 3) uint32: the floats' bits, row 0 on top"""
    data = open(path, "rb").read()
    magic, size, scale, body = data.split(b"\n", 3)
    assert magic == b"PF" and scale == b"-1.0", (magic, scale)
    w, h = (int(v) for v in size.split())
    assert len(body) == w * h * 12
    return np.frombuffer(body, dtype="<u4").reshape(h, w, 3)[::-1].astype(np.uint32)


def read_png16(path):
    """(h, w, 3) uint16 of a colour-type-2, 16-bit PNG, and the list of the rows' filter types: chunks, CRCs, zlib, every filter undone here"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, ihdr, ended = 8, b"", None, False
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            ended = True
        at += 12 + n
    assert ended and at == len(data)
    w, h, depth, colour, comp, filt, interlace = ihdr
    assert (depth, colour, comp, filt, interlace) == (16, 2, 0, 0, 0), ihdr
    raw = zlib.decompress(idat)
    stride, bpp = w * 6, 6
    assert len(raw) == (stride + 1) * h
    rows, filters = [], []
    prev = bytearray(stride)
    for j in range(h):
        line = raw[j * (stride + 1):(j + 1) * (stride + 1)]
        f, cur = line[0], bytearray(line[1:])
        filters.append(f)
        assert f <= 4
        for x in range(stride):
            a = cur[x - bpp] if x >= bpp else 0
            b = prev[x]
            c = prev[x - bpp] if x >= bpp else 0
            if f == 1:
                pred = a
            elif f == 2:
                pred = b
            elif f == 3:
                pred = (a + b) >> 1
            elif f == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
            else:
                pred = 0
            cur[x] = (cur[x] + pred) & 0xFF
        rows.append(bytes(cur))
        prev = cur
    return np.frombuffer(b"".join(rows), dtype=">u2").reshape(h, w, 3).astype(np.uint16), filters
