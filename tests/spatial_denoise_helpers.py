"""Shared by the spatial-variance tests (not a test module): the normative definition of include/rt_amd.h "spatial variance" in numpy —
the prepare step that takes a pixel's variance from the spread of its neighbours' values, plain and guided — on top of the restatements
the other denoise tests use, which are imported unchanged: the iterations are denoise_helpers.iterate and albedo_helpers.iterate, and at
or above the threshold the whole filter is live_denoise_helpers.denoise_mean / denoise_albedo_mean.

As there, every line is one elementwise f64 operation (numpy neither contracts a * b + c nor replaces a division by a reciprocal
multiply), a window member that is skipped adds nothing (np.where keeps the old value: not even a zero is added), and max(a, b) is
b > a ? b : a."""
import numpy as np

import albedo_helpers
import denoise_helpers
import live_denoise_helpers as ldh
from denoise_helpers import _shifted

DEFAULTS = dict(spatial_below=2, window_radius=1)


def _max(a, b):
    return np.where(b > a, b, a)


def _spread(C0, valid, R):
    """V0 (h, w) of the valid pixels (-1 elsewhere) from C0 (h, w, 3): the two passes over the (2R + 1)^2 window, dy outer, dx inner"""
    h, w = valid.shape
    with np.errstate(all="ignore"):
        cnt = np.zeros((h, w))
        s1 = [np.zeros((h, w)) for _ in range(3)]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                ok = _shifted(valid, dy, dx, False)
                cnt = np.where(ok, cnt + 1.0, cnt)
                for c in range(3):
                    s1[c] = np.where(ok, s1[c] + _shifted(C0[:, :, c], dy, dx, 0.0), s1[c])
        mu = [s1[c] / cnt for c in range(3)]
        s2 = [np.zeros((h, w)) for _ in range(3)]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                ok = _shifted(valid, dy, dx, False)
                for c in range(3):
                    t = _shifted(C0[:, :, c], dy, dx, 0.0) - mu[c]
                    tt = t * t
                    s2[c] = np.where(ok, s2[c] + tt, s2[c])
        v = [np.where(cnt >= 2.0, s2[c] / (cnt - 1.0), 0.0) for c in range(3)]
        V = _max(_max(v[0], v[1]), v[2])
    return np.where(valid, V, -1.0)


def prepare_spatial(M, R=DEFAULTS["window_radius"]):
    """(C0 (h, w, 3), V0 (h, w), valid (h, w))"""
    M = np.asarray(M, dtype=np.float64)
    valid = np.isfinite(M).all(axis=2)
    return M, _spread(M, valid, R), valid


def prepare_albedo_spatial(M, A, albedo_floor, R=DEFAULTS["window_radius"]):
    """(C0 (h, w, 3), V0 (h, w), valid (h, w), a (h, w, 3), d (h, w, 3)); A: the albedo MEANS"""
    M, a = np.asarray(M, dtype=np.float64), np.asarray(A, dtype=np.float64)
    valid = np.isfinite(M).all(axis=2) & np.isfinite(a).all(axis=2)
    with np.errstate(all="ignore"):
        d = _max(a, np.float64(albedo_floor))
        I = M / d
    C0 = np.where(valid[:, :, None], I, M)
    return C0, _spread(C0, valid, R), valid, a, d


def denoise_mean_spatial(M, M2, n, spatial_below=DEFAULTS["spatial_below"], window_radius=DEFAULTS["window_radius"],
                         iterations=ldh.DEFAULTS["iterations"], sigma=ldh.DEFAULTS["sigma"], eps=ldh.DEFAULTS["eps"]):
    """C_K, an (h, w, 3) float64 frame; M2 is not looked at where n < spatial_below (None will do)"""
    if n >= spatial_below:
        return ldh.denoise_mean(M, M2, n, iterations=iterations, sigma=sigma, eps=eps)
    C, V, valid = prepare_spatial(M, window_radius)
    for k in range(iterations):
        C, V = denoise_helpers.iterate(C, V, valid, 1 << k, sigma, eps)
    return C


def denoise_albedo_mean_spatial(M, M2, n, A, spatial_below=DEFAULTS["spatial_below"], window_radius=DEFAULTS["window_radius"],
                                iterations=ldh.ALBEDO_DEFAULTS["iterations"], sigma=ldh.ALBEDO_DEFAULTS["sigma"], eps=ldh.ALBEDO_DEFAULTS["eps"],
                                sigma_albedo=ldh.ALBEDO_DEFAULTS["sigma_albedo"], albedo_floor=ldh.ALBEDO_DEFAULTS["albedo_floor"]):
    """out, an (h, w, 3) float64 frame: C_K * d for a valid pixel, m for any other"""
    if n >= spatial_below:
        return ldh.denoise_albedo_mean(M, M2, n, A, iterations=iterations, sigma=sigma, eps=eps, sigma_albedo=sigma_albedo, albedo_floor=albedo_floor)
    C, V, valid, a, d = prepare_albedo_spatial(M, A, albedo_floor, window_radius)
    for k in range(iterations):
        C, V = albedo_helpers.iterate(C, V, valid, a, 1 << k, sigma, eps, sigma_albedo)
    with np.errstate(all="ignore"):
        return np.where(valid[:, :, None], C * d, C)


display = denoise_helpers.display
