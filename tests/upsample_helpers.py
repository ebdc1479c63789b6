"""The definition of include/rt_amd.h "guided upsampling" restated in numpy, one rounded f64 operation per step (numpy does not contract a
multiplication and an addition of two separate ufunc calls), the camera of the small frame restated in Python floats, and the inputs the
upsampling tests share."""
import numpy as np

DEFAULTS = dict(factor=2, sigma_edge=0.5, sigma_albedo=0.5, albedo_floor=1e-3)
FACTORS = (2, 3, 4)
GUIDE_SETS = ("none", "edge", "albedo", "both")
# tools/upsample_sweep.py's figure (DESIGN.md section 5 "Upsampling") for the Cornell box at 64 x 64, F = 2, 16 spp low (seed 5), albedo
# and ID guides at 4 spp, the defaults, not denoised first, against the 1024-spp mean of seed 77 — as the sweep prints it
SWEEP_CORNELL_F2_BOTH = "1.2013e-01"
# full sizes of the bit-for-bit tests: 1 x 1 and 2 x 2 are smaller than a block (w < F), 13 x 7 and 5 x 3 leave a ragged last block, and
# 65 x 17 is one pixel past two tiles of 32 x 8 on both axes
HOST_SHAPES = [(13, 7), (1, 1), (2, 2), (5, 3), (65, 17)]
# ... and on the device: many tiles on one axis, whole tiles, and ragged tiles on both axes with the low halo crossing workgroup tiles
GPU_SHAPES = HOST_SHAPES + [(130, 9), (64, 64), (257, 33)]


def low_size(n, F):
    return (n + F - 1) // F


def hmax(a, b):
    """the header's max(a, b) = (b > a ? b : a)"""
    with np.errstate(invalid="ignore"):
        return np.where(b > a, b, a)


def camera_scaled(cam, F):
    """rt_camera_scaled on a dict of Python floats: {"w", "h", "p00": [3], "du": [3], "dv": [3]} -> the same keys"""
    f = float(F)
    out = dict(w=low_size(cam["w"], F), h=low_size(cam["h"], F), p00=[], du=[], dv=[])
    for p00, du, dv in zip(cam["p00"], cam["du"], cam["dv"]):
        du2, dv2 = f * du, f * dv
        corner = p00 - (0.5 * (du + dv))
        out["p00"].append(corner + (0.5 * (du2 + dv2)))
        out["du"].append(du2)
        out["dv"].append(dv2)
    return out


def block_mean(full, F):
    """per low pixel: acc = +0.0, the in-frame pixels of its F x F block added rows outer, divided by their count as a double"""
    h, w = full.shape[:2]
    lh, lw = low_size(h, F), low_size(w, F)
    acc = np.zeros((lh, lw, 3))
    count = np.zeros((lh, lw))
    with np.errstate(all="ignore"):
        for dy in range(F):
            for dx in range(F):
                sub = full[dy::F, dx::F]
                nj, ni = sub.shape[:2]
                acc[:nj, :ni] = acc[:nj, :ni] + sub
                count[:nj, :ni] += 1.0
        return acc / count[..., None]


def stop(p, q, sigma):
    """d = max over the channels of |p_c - q_c|; z = d / sigma; t = 1 - z * z; t > 0 ? t * t : 0"""
    with np.errstate(all="ignore"):
        d = np.abs(p - q)
        dg = hmax(hmax(d[..., 0], d[..., 1]), d[..., 2])
        z = dg / sigma
        t = 1.0 - z * z
        return np.where(t > 0.0, t * t, 0.0)


def footprint(n, F):
    """per full-size coordinate: i0 and rx"""
    t = 2 * np.arange(n, dtype=np.int64) + 1 - F
    i0 = t // (2 * F)              # floor division
    return i0, t - 2 * F * i0


def low_records(low, spp, size, albedo_sum=None, albedo_spp=0, edge_sum=None, edge_spp=0, *, factor=2, albedo_floor=1e-3):
    """(R, valid, a, a_low, g, g_low): the prepare step"""
    w, h = size
    F = factor
    low = np.asarray(low, dtype=np.float64)
    assert low.shape == (low_size(h, F), low_size(w, F), 3)
    with np.errstate(all="ignore"):
        C = low * (np.float64(1.0) / np.float64(spp))
        valid = np.isfinite(C).all(axis=-1)
        a = a_low = g = g_low = None
        R = C
        if albedo_sum is not None:
            a = np.asarray(albedo_sum, dtype=np.float64) / np.float64(albedo_spp)
            a_low = block_mean(a, F)
            valid = valid & np.isfinite(a_low).all(axis=-1)
            R = C / hmax(a_low, np.float64(albedo_floor))
        if edge_sum is not None:
            g = np.asarray(edge_sum, dtype=np.float64) / np.float64(edge_spp)
            g_low = block_mean(g, F)
            valid = valid & np.isfinite(g_low).all(axis=-1)
    return R, valid, a, a_low, g, g_low


def upsample(low, spp, size, albedo_sum=None, albedo_spp=0, edge_sum=None, edge_spp=0, *, factor=2, sigma_edge=0.5, sigma_albedo=0.5,
             albedo_floor=1e-3, reverse=False):
    """the (h, w, 3) frame rt_upsample_device defines (reverse: the taps summed in the opposite order — NOT the definition, the
    accumulation-order test's foil)"""
    w, h = size
    F = factor
    lh, lw = low_size(h, F), low_size(w, F)
    R, valid, a, a_low, g, g_low = low_records(low, spp, size, albedo_sum, albedo_spp, edge_sum, edge_spp, factor=F, albedo_floor=albedo_floor)
    i0, rx = footprint(w, F)
    j0, ry = footprint(h, F)
    sw = np.zeros((h, w))
    sc = np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        for dj in (range(2, -2, -1) if reverse else range(-1, 3)):
            J = j0 + dj
            wy = (4 * F - np.abs(2 * F * dj - ry)).astype(np.float64) / np.float64(4 * F)
            Jc = np.clip(J, 0, lh - 1)
            for di in (range(2, -2, -1) if reverse else range(-1, 3)):
                I = i0 + di
                wx = (4 * F - np.abs(2 * F * di - rx)).astype(np.float64) / np.float64(4 * F)
                Ic = np.clip(I, 0, lw - 1)
                at = (Jc[:, None], Ic[None, :])
                ok = ((J >= 0) & (J < lh))[:, None] & ((I >= 0) & (I < lw))[None, :] & valid[at]
                ws = wy[:, None] * wx[None, :]
                if a is not None and g is not None:
                    wt = ws * (stop(a, a_low[at], sigma_albedo) * stop(g, g_low[at], sigma_edge))
                elif a is not None:
                    wt = ws * stop(a, a_low[at], sigma_albedo)
                elif g is not None:
                    wt = ws * stop(g, g_low[at], sigma_edge)
                else:
                    wt = ws
                sw = np.where(ok, sw + wt, sw)                                       # a skipped tap adds nothing at all
                sc = np.where(ok[..., None], sc + (wt[..., None] * R[at]), sc)
        own = R[(np.arange(h) // F)[:, None], (np.arange(w) // F)[None, :]]
        some = sw > 0.0
        r = np.where(some[..., None], sc / np.where(some, sw, 1.0)[..., None], own)
        return r * hmax(a, np.float64(albedo_floor)) if a is not None else r


def guides_for(kind, albedo, edge):
    """the keyword arguments of a guide set: kind is one of GUIDE_SETS; albedo and edge are (sums, spp)"""
    kw = {}
    if kind in ("albedo", "both"):
        kw.update(albedo_sum=albedo[0], albedo_spp=albedo[1])
    if kind in ("edge", "both"):
        kw.update(edge_sum=edge[0], edge_spp=edge[1])
    return kw


PALETTE = np.array([(0.5 * (q % 3), 0.5 * ((q // 3) % 3), 0.5 * (q // 9)) for q in range(1, 27)])   # the surface-ID colours


def inputs(w, h, F, seed=0, special=False):
    """(low sums, spp, (albedo sums, albedo_spp), (edge sums, edge_spp)) for a full size w x h: a low frame of mixed magnitude
    (1e-6 .. 1e6, some channels negative), an albedo frame in [0, 1] with patches under the floor, an ID frame of palette colours in
    random patches with some anti-aliased (mixed) pixels; `special`: scattered NaN and +-inf in the low frame and in both guides"""
    rng = np.random.default_rng(4000 + 97 * seed + F)
    lh, lw = low_size(h, F), low_size(w, F)
    spp, n_a, n_e = 5, 3, 4
    low = 10.0 ** rng.uniform(-6.0, 6.0, size=(lh, lw, 3))
    low = np.where(rng.random((lh, lw, 3)) < 0.1, -low, low)
    albedo = rng.uniform(0.0, 1.0, size=(h, w, 3)) * n_a
    albedo[rng.random((h, w)) < 0.1] = 1e-5 * n_a
    coarse = rng.integers(0, 4, size=(h // 3 + 1, w // 3 + 1))
    ids = PALETTE[np.repeat(np.repeat(coarse, 3, axis=0), 3, axis=1)[:h, :w]]
    mixed = rng.random((h, w)) < 0.15
    ids = np.where(mixed[..., None], 0.5 * (ids + PALETTE[rng.integers(0, 26, size=(h, w))]), ids) * n_e
    if special:
        for frame in (low, albedo, ids):
            flat = frame.reshape(-1, 3)
            for value in (np.nan, np.inf, -np.inf):
                flat[rng.integers(0, len(flat), size=max(1, len(flat) // 30)), rng.integers(0, 3)] = value
    return np.ascontiguousarray(low), spp, (np.ascontiguousarray(albedo), n_a), (np.ascontiguousarray(ids), n_e)


def step_case(w, h, F, x0):
    """The synthetic step: the truth is 1 left of column x0 and 0 from it on; the low frame is its exact block mean (means: spp 1); the
    ID guide is one palette colour on each side.  Returns (truth (h, w, 3), low, edge sums)."""
    truth = np.zeros((h, w, 3))
    truth[:, :x0] = 1.0
    low = block_mean(truth, F)
    edge = np.where((np.arange(w) < x0)[None, :, None], PALETTE[3], PALETTE[7]) * np.ones((h, w, 1))
    return truth, np.ascontiguousarray(low), np.ascontiguousarray(edge)


def same_bits(a, b):
    """the same doubles bit for bit; a NaN matches any NaN (the sign and payload of a NaN that an operation makes, inf - inf say, are
    the processor's choice and differ between host and device), but only in the same place"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])
