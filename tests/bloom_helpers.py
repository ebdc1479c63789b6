"""The definition of include/rt_amd.h "bloom" restated in numpy, one rounded f64 operation per step (numpy does not contract a
multiplication and an addition of two separate ufunc calls), and the inputs the bloom tests share."""
import numpy as np

H = (0.0625, 0.25, 0.375, 0.25, 0.0625)          # the B3-spline taps, d = -2 .. 2
DEFAULTS = dict(levels=5, threshold=1.0, strength=0.25)
# the frames of the bit-for-bit tests: (w, h, levels)
SHAPES = [(1, 1, 4), (1, 7, 4), (7, 1, 4), (5, 3, 4), (17, 9, 4), (64, 16, 4), (65, 17, 4),   # 64 x 16: one fused tile exactly, and one past it
          (130, 70, 6),                                                                      # stride 32: most taps of edge pixels are out of frame
          (40, 24, 8)]                                                                       # stride 128 exceeds the frame: the centre tap only
LONG = [(256, 8, 4), (8, 256, 4)]                                                            # long rows and long columns


def means(values, spp, spp_map=None):
    """m = S * (1.0 / (double)n)"""
    values = np.asarray(values, dtype=np.float64)
    if spp_map is None:
        return values * (np.float64(1.0) / np.float64(spp))
    return values * (np.float64(1.0) / np.asarray(spp_map, dtype=np.float64))[..., None]


def luminance(m):
    return ((0.2126 * m[..., 0]) + (0.7152 * m[..., 1])) + (0.0722 * m[..., 2])


def bright(m, threshold):
    """B0: m * ((L - threshold) / L) where the pixel is a source, +0.0 elsewhere"""
    with np.errstate(all="ignore"):
        L = luminance(m)
        ok = np.isfinite(m).all(axis=-1) & np.isfinite(L) & (L > threshold)
        k = np.where(ok, (L - threshold) / np.where(ok, L, 1.0), 0.0)
        return np.where(ok[..., None], m * k[..., None], 0.0)


def taps(B, stride, axis):
    """acc = +0.0; for d = -2 .. 2 in order, acc = acc + (h[d] * B(shifted by stride * d along axis)), taps outside the frame skipped"""
    n = B.shape[axis]
    acc = np.zeros_like(B)
    for d in range(-2, 3):
        off = stride * d
        lo, hi = max(0, -off), min(n, n - off)     # the destinations whose tap lies inside
        if lo >= hi:
            continue
        dst = [slice(None)] * B.ndim
        src = [slice(None)] * B.ndim
        dst[axis], src[axis] = slice(lo, hi), slice(lo + off, hi + off)
        with np.errstate(all="ignore"):
            acc[tuple(dst)] = acc[tuple(dst)] + (H[d + 2] * B[tuple(src)])
    return acc


def level_frames(B0, levels):
    """[B_1, ..., B_K]: each level the horizontal accumulation (axis 1 of an (h, w, 3) frame), then the vertical one over it"""
    out, B = [], B0
    for k in range(levels):
        B = taps(taps(B, 1 << k, 1), 1 << k, 0)
        out.append(B)
    return out


def accumulate(frames):
    """A_K = (((+0.0 + B_1) + B_2) + ...) + B_K"""
    A = np.zeros_like(frames[0])
    for B in frames:
        with np.errstate(all="ignore"):
            A = A + B
    return A


def bloom(values, spp, spp_map=None, *, levels=5, threshold=1.0, strength=0.25):
    m = means(values, spp, spp_map)
    A = accumulate(level_frames(bright(m, threshold), levels))
    with np.errstate(all="ignore"):
        g = A / np.float64(levels)
        return m + (strength * g)


def blur_2d(B, stride):
    """one level as a 25-tap 2-D sum, rows outer, weights h[dj] * h[di]: NOT the definition (the separable test's foil)"""
    h, w = B.shape[:2]
    acc = np.zeros_like(B)
    for dj in range(-2, 3):
        for di in range(-2, 3):
            oj, oi = stride * dj, stride * di
            j0, j1, i0, i1 = max(0, -oj), min(h, h - oj), max(0, -oi), min(w, w - oi)
            if j0 >= j1 or i0 >= i1:
                continue
            acc[j0:j1, i0:i1] = acc[j0:j1, i0:i1] + ((H[dj + 2] * H[di + 2]) * B[j0 + oj:j1 + oj, i0 + oi:i1 + oi])
    return acc


def frame(w, h, seed=0, special=True):
    """an (h, w, 3) frame of mixed magnitude (1e-12 .. 1e6), some channels negative, and — `special` — -0.0 values and scattered NaN
    and +-inf pixels; seeded"""
    rng = np.random.default_rng(1000 + seed)
    f = 10.0 ** rng.uniform(-12.0, 6.0, size=(h, w, 3))
    f = np.where(rng.random((h, w, 3)) < 0.15, -f, f)
    if special:
        n = w * h
        flat = f.reshape(n, 3)
        flat[rng.random(n) < 0.05, 1] = -0.0
        for value in (np.nan, np.inf, -np.inf):
            flat[rng.integers(0, n, size=max(1, n // 40)), rng.integers(0, 3)] = value
    return np.ascontiguousarray(f)


def spp_map_for(w, h, seed=0):
    return np.random.default_rng(2000 + seed).integers(1, 40, size=(h, w)).astype(np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
