"""Shared by the tests of the edge guide on the means, spatial-variance and views routes (not a test module): the normative
definitions of include/rt_amd.h "edge guide on every route" in numpy, built from the restatements the other denoise tests use, which
are imported unchanged — the iterations and the stop are guided_helpers.iterate / _stop, the means-form and spatial prepares are
live_denoise_helpers' and spatial_denoise_helpers', and a views stack is guided_helpers.denoise_guided per view.

As there, every line is one elementwise f64 operation (numpy neither contracts a * b + c nor replaces a division by a reciprocal
multiply), a window pixel that is no member adds nothing (np.where keeps the old value), and max(a, b) is b > a ? b : a.  With A None
a filter is the plain one with the edge stop; otherwise the albedo-guided one with it.  E is always a frame of MEANS here."""
import numpy as np

import guided_helpers as gh
import live_denoise_helpers as ldh
import spatial_denoise_helpers as sdh
from denoise_helpers import _shifted

DEFAULTS = gh.DEFAULTS
SPATIAL_DEFAULTS = sdh.DEFAULTS
display = gh.display


def _max(a, b):
    return np.where(b > a, b, a)


# ---- the means form ----
def prepare_guided_mean(M, M2, n, E, A=None, albedo_floor=DEFAULTS["albedo_floor"]):
    """(C0, V0, valid, g, a, d): live_denoise_helpers' prepare with `valid` also asking for a finite E; C0 and V0 untouched by E"""
    g = np.asarray(E, dtype=np.float64)
    fin = np.isfinite(g).all(axis=2)
    if A is None:
        C, V, valid = ldh.prepare_mean(M, M2, n)
        a = d = None
        M = C
    else:
        C, V, valid, a, d = ldh.prepare_albedo_mean(M, M2, n, A, albedo_floor)
        M = np.asarray(M, dtype=np.float64)
    valid = valid & fin
    return np.where(valid[:, :, None], C, M), np.where(valid, V, -1.0), valid, g, a, d


def _finish(C, V, valid, g, a, d, iterations, sigma, eps, sigma_albedo, sigma_edge):
    for k in range(iterations):
        C, V = gh.iterate(C, V, valid, g, a, 1 << k, sigma, eps, sigma_albedo, sigma_edge)
    if a is None:
        return C
    with np.errstate(all="ignore"):
        return np.where(valid[:, :, None], C * d, C)


def denoise_guided_mean(M, M2, n, E, A=None, iterations=DEFAULTS["iterations"], sigma=DEFAULTS["sigma"], eps=DEFAULTS["eps"],
                        sigma_albedo=DEFAULTS["sigma_albedo"], albedo_floor=DEFAULTS["albedo_floor"], sigma_edge=DEFAULTS["sigma_edge"]):
    """out, an (h, w, 3) float64 frame: C_K (with an albedo frame: C_K * d) for a valid pixel, m for any other"""
    C, V, valid, g, a, d = prepare_guided_mean(M, M2, n, E, A, albedo_floor)
    return _finish(C, V, valid, g, a, d, iterations, sigma, eps, sigma_albedo, sigma_edge)


# ---- the spatial form ----
def _member(g, dy, dx, sigma_edge):
    """q = p + (dx, dy) passes p's edge stop: tg = 1 - (dg / sigma_edge)^2 > 0 (a NaN anywhere: no member)"""
    gq = _shifted(g, dy, dx, 0.0)
    dg = _max(_max(np.abs(g[:, :, 0] - gq[:, :, 0]), np.abs(g[:, :, 1] - gq[:, :, 1])), np.abs(g[:, :, 2] - gq[:, :, 2]))
    z = dg / sigma_edge
    tg = 1.0 - z * z
    return tg > 0.0


def _spread_guided(C0, valid, g, R, sigma_edge):
    """spatial_denoise_helpers._spread over the members only"""
    h, w = valid.shape
    with np.errstate(all="ignore"):
        cnt = np.zeros((h, w))
        s1 = [np.zeros((h, w)) for _ in range(3)]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                ok = _shifted(valid, dy, dx, False) & _member(g, dy, dx, sigma_edge)
                cnt = np.where(ok, cnt + 1.0, cnt)
                for c in range(3):
                    s1[c] = np.where(ok, s1[c] + _shifted(C0[:, :, c], dy, dx, 0.0), s1[c])
        mu = [s1[c] / cnt for c in range(3)]
        s2 = [np.zeros((h, w)) for _ in range(3)]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                ok = _shifted(valid, dy, dx, False) & _member(g, dy, dx, sigma_edge)
                for c in range(3):
                    t = _shifted(C0[:, :, c], dy, dx, 0.0) - mu[c]
                    tt = t * t
                    s2[c] = np.where(ok, s2[c] + tt, s2[c])
        v = [np.where(cnt >= 2.0, s2[c] / (cnt - 1.0), 0.0) for c in range(3)]
        V = _max(_max(v[0], v[1]), v[2])
    return np.where(valid, V, -1.0)


def prepare_guided_spatial(M, E, A=None, albedo_floor=DEFAULTS["albedo_floor"], R=SPATIAL_DEFAULTS["window_radius"], sigma_edge=DEFAULTS["sigma_edge"]):
    """(C0, V0, valid, g, a, d)"""
    M, g = np.asarray(M, dtype=np.float64), np.asarray(E, dtype=np.float64)
    valid = np.isfinite(M).all(axis=2) & np.isfinite(g).all(axis=2)
    if A is None:
        a = d = None
        C0 = M
    else:
        a = np.asarray(A, dtype=np.float64)
        valid = valid & np.isfinite(a).all(axis=2)
        with np.errstate(all="ignore"):
            d = _max(a, np.float64(albedo_floor))
            C0 = np.where(valid[:, :, None], M / d, M)
    return C0, _spread_guided(C0, valid, g, R, sigma_edge), valid, g, a, d


def denoise_guided_mean_spatial(M, M2, n, E, A=None, spatial_below=SPATIAL_DEFAULTS["spatial_below"], window_radius=SPATIAL_DEFAULTS["window_radius"],
                                iterations=DEFAULTS["iterations"], sigma=DEFAULTS["sigma"], eps=DEFAULTS["eps"],
                                sigma_albedo=DEFAULTS["sigma_albedo"], albedo_floor=DEFAULTS["albedo_floor"], sigma_edge=DEFAULTS["sigma_edge"]):
    """out, an (h, w, 3) float64 frame; M2 is not looked at where n < spatial_below (None will do)"""
    if n >= spatial_below:
        return denoise_guided_mean(M, M2, n, E, A, iterations, sigma, eps, sigma_albedo, albedo_floor, sigma_edge)
    C, V, valid, g, a, d = prepare_guided_spatial(M, E, A, albedo_floor, window_radius, sigma_edge)
    return _finish(C, V, valid, g, a, d, iterations, sigma, eps, sigma_albedo, sigma_edge)


# ---- the views form ----
def denoise_guided_views(S, Q, n, E, n_e, A=None, n_a=0, **kw):
    """(n_views, h, w, 3): guided_helpers.denoise_guided on each view's frames (E, A: sums, as on the sums route)"""
    return np.stack([gh.denoise_guided(S[v], Q[v], n, E[v], n_e, None if A is None else A[v], n_a, **kw) for v in range(len(S))])


# ---- inputs ----
def synthetic_edge_mean(w, h, seed):
    """guided_helpers.synthetic_edges' frame as MEANS: E / n_e of that generator"""
    E, n_e = gh.synthetic_edges(w, h, seed)
    with np.errstate(all="ignore"):
        return E / float(n_e)


def constant_guide(w, h, value=(0.5, 1.0, 0.0)):
    return np.broadcast_to(np.asarray(value, dtype=np.float64), (h, w, 3)).copy()


def step_frames(w, h):
    """(M, E): the two-surface step — the left half 0.25 and the right 0.75 (dyadic: every in-order sum of up to 49 of either is
    exact), the guide two palette colours split at the same column"""
    M = np.empty((h, w, 3))
    M[:, : w // 2] = 0.25
    M[:, w // 2:] = 0.75
    E = np.empty((h, w, 3))
    E[:, : w // 2] = gh.palette(1)
    E[:, w // 2:] = gh.palette(2)
    return M, E
