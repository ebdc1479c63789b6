"""Shared by the denoise tests (not a test module): the normative definition of include/rt_amd.h "denoise" in numpy, vectorised over
pixels with the taps in the stated order, and the frames the tests feed it.

Every line below is one elementwise f64 operation (numpy neither contracts a * b + c nor replaces a division by a reciprocal
multiply), a tap that is skipped leaves its pixel's sums untouched (np.where keeps the old value: nothing is added, not even a
zero), and max(a, b) is b > a ? b : a."""
import numpy as np

from live_helpers import oracle_samples  # noqa: F401  (the tests build moments from the oracle's single-sample frames)

G3 = (0.25, 0.5, 0.25)
H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEFAULTS = dict(iterations=4, sigma=4.0, eps=1e-6)


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` where that is out of frame"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        out[yd, xd] = a[ys, xs]
    return out


def prepare(S, Q, n):
    """(C0 (h, w, 3), V0 (h, w), valid (h, w)); n: an int or an (h, w) integer array"""
    S = np.asarray(S, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    h, w = S.shape[:2]
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), (h, w))
    dn = n.astype(np.float64)
    with np.errstate(all="ignore"):
        m = S / dn[:, :, None]
        valid = (n >= 2) & np.isfinite(S).all(axis=2) & np.isfinite(Q).all(axis=2)
        v = (Q - S * m) / (dn - 1.0)[:, :, None]
        vmax = v[:, :, 0]
        vmax = np.where(v[:, :, 1] > vmax, v[:, :, 1], vmax)
        vmax = np.where(v[:, :, 2] > vmax, v[:, :, 2], vmax)
        vmax = np.where(0.0 > vmax, 0.0, vmax)
        V = vmax / dn
    return m, np.where(valid, V, -1.0), valid


def iterate(C, V, valid, stride, sigma, eps):
    h, w = V.shape
    with np.errstate(all="ignore"):
        L = ((C[:, :, 0] + C[:, :, 1]) + C[:, :, 2]) / 3.0
        gs, ws = np.zeros((h, w)), np.zeros((h, w))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = _shifted(valid, dy, dx, False)
                k = G3[dy + 1] * G3[dx + 1]
                gs = np.where(ok, gs + k * _shifted(V, dy, dx, 0.0), gs)
                ws = np.where(ok, ws + k, ws)
        G = gs / ws
        sd = np.sqrt(G)
        den = sigma * sd + eps
        sw, sv = np.zeros((h, w)), np.zeros((h, w))
        sc = [np.zeros((h, w)) for _ in range(3)]
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                oy, ox = dy * stride, dx * stride
                ok = _shifted(valid, oy, ox, False)
                x = np.abs(L - _shifted(L, oy, ox, 0.0)) / den
                t = 1.0 - x * x
                e = np.where(t > 0.0, t * t, 0.0)
                wq = (H5[dy + 2] * H5[dx + 2]) * e
                sw = np.where(ok, sw + wq, sw)
                for c in range(3):
                    sc[c] = np.where(ok, sc[c] + wq * _shifted(C[:, :, c], oy, ox, 0.0), sc[c])
                sv = np.where(ok, sv + (wq * wq) * _shifted(V, oy, ox, 0.0), sv)
        Cn = np.stack([np.where(valid, sc[c] / sw, C[:, :, c]) for c in range(3)], axis=2)
        Vn = np.where(valid, sv / (sw * sw), V)
    return Cn, Vn


def denoise(S, Q, n, iterations=4, sigma=4.0, eps=1e-6):
    """C_K, an (h, w, 3) float64 frame"""
    C, V, valid = prepare(S, Q, n)
    for k in range(iterations):
        C, V = iterate(C, V, valid, 1 << k, sigma, eps)
    return C


def display(rt, mean):
    """the RGBA8 bytes of a frame of means: the host library's color_to_rgb at spp 1, alpha 255"""
    h, w = mean.shape[:2]
    out = np.full((h, w, 4), 255, dtype=np.uint8)
    out[:, :, :3] = rt.resolve_rgb8_host(w, h, 1, mean)
    return out


def moments(colours, shape):
    """(S, Q) as (h, w, 3): the in-order sums of the samples and of their squares (each product rounded, then added)"""
    S, Q = np.zeros_like(colours[0]), np.zeros_like(colours[0])
    for c in colours:
        S = S + c
        Q = Q + c * c
    return S.reshape(shape), Q.reshape(shape)


def synthetic(w, h, seed):
    """(S, Q, spp, spp_map): moments of `spp` made-up samples per pixel — noisy gradients, a block of exactly zero variance beside a
    different constant (the hard edge at sd = 0), a few NaN and +-inf entries in S or Q — and an spp map that mixes values, with
    0, 1 and 2 among them.  The moments stay as they are under the map: the definition reads them as whatever n says."""
    rng = np.random.default_rng(seed)
    spp = 8
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.2 + 0.6 * xx / max(w - 1, 1), 0.3 + 0.5 * yy / max(h - 1, 1), 0.5 + 0.0 * xx], axis=2)
    samples = base[None] * (1.0 + 0.5 * rng.standard_normal((spp, h, w, 3)))
    bx, by = w // 3, h // 3
    samples[:, by:by + max(h // 3, 1), bx:bx + max(w // 6, 1), :] = 0.25        # zero variance ...
    samples[:, by:by + max(h // 3, 1), bx + max(w // 6, 1):bx + 2 * max(w // 6, 1), :] = 0.75  # ... next to another constant
    S, Q = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for s in range(spp):
        S = S + samples[s]
        Q = Q + samples[s] * samples[s]
    if w * h >= 15:
        bad = rng.choice(w * h, size=min(6, w * h // 5), replace=False)
        for k, p in enumerate(bad):
            (S if k % 2 else Q).reshape(-1, 3)[p, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    spp_map = rng.choice(np.array([0, 1, 2, 3, 8, 8, 8, 16, 31], dtype=np.int32), size=(h, w))
    if w * h >= 3:
        spp_map.reshape(-1)[:3] = (0, 1, 2)
    return S, Q, spp, spp_map.astype(np.int32)
