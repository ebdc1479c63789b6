"""Shared by the live-denoise tests (not a test module): the normative definitions of include/rt_amd.h "live denoise" in numpy — the
running mean with Welford's M2 beside it, and the means-form prepare step of the two filters — on top of the restatements the live,
denoise and albedo-guided denoise tests already use, which are imported unchanged: the recurrence of the mean is live_helpers.fold's,
the iterations are denoise_helpers.iterate and albedo_helpers.iterate.

As there, every line is one elementwise f64 operation (numpy neither contracts a * b + c nor replaces a division by a reciprocal
multiply) and max(a, b) is b > a ? b : a."""
import numpy as np

import albedo_helpers
import denoise_helpers
import live_helpers  # noqa: F401  (oracle_samples, fold: the tests hold fold_moments' mean to fold)

DEFAULTS = denoise_helpers.DEFAULTS
ALBEDO_DEFAULTS = albedo_helpers.DEFAULTS


# ---- the reduction ----
def fold_moments(colours, mean=None, m2=None, first=0, terms=None):
    """(m, M2) after the samples `colours` (sample s = first, first + 1, ...):  d = c - m;  m' = m + d / (s + 1);  M2 = M2 + d * (c - m');
    m = m'.  `mean`, `m2`: the values after `first` samples (+0.0 if None).  `terms`, a list: every d * (c - m') is appended to it."""
    zero = np.zeros_like(np.asarray(colours[0], dtype=np.float64))
    m = zero.copy() if mean is None else np.array(mean, dtype=np.float64)
    q = zero.copy() if m2 is None else np.array(m2, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k, c in enumerate(colours):
            c = np.asarray(c, dtype=np.float64)
            d = c - m
            step = d / np.float64(first + k + 1)
            m1 = m + step
            t = c - m1
            p = d * t
            q = q + p
            m = m1
            if terms is not None:
                terms.append(p)
    return m, q


def sums_variance(colours):
    """(v, S, Q): the sums form's (Q - S * m) / (n - 1) over the samples, m = S / n"""
    S, Q = denoise_helpers.moments(colours, np.asarray(colours[0]).shape)
    n = float(len(colours))
    m = S / n
    return (Q - S * m) / (n - 1.0), S, Q


# ---- the means-form filters ----
def _max(a, b):
    return np.where(b > a, b, a)


def prepare_mean(M, M2, n):
    """(C0 (h, w, 3), V0 (h, w), valid (h, w)); n: the uniform sample count"""
    M, M2 = np.asarray(M, dtype=np.float64), np.asarray(M2, dtype=np.float64)
    dn = np.float64(n)
    with np.errstate(all="ignore"):
        valid = np.full(M.shape[:2], int(n) >= 2) & np.isfinite(M).all(axis=2) & np.isfinite(M2).all(axis=2)
        v = M2 / (dn - 1.0)
        vmax = _max(_max(_max(v[:, :, 0], v[:, :, 1]), v[:, :, 2]), 0.0)
        V = vmax / dn
    return M, np.where(valid, V, -1.0), valid


def denoise_mean(M, M2, n, iterations=DEFAULTS["iterations"], sigma=DEFAULTS["sigma"], eps=DEFAULTS["eps"]):
    """C_K, an (h, w, 3) float64 frame"""
    C, V, valid = prepare_mean(M, M2, n)
    for k in range(iterations):
        C, V = denoise_helpers.iterate(C, V, valid, 1 << k, sigma, eps)
    return C


def prepare_albedo_mean(M, M2, n, A, albedo_floor):
    """(C0 (h, w, 3), V0 (h, w), valid (h, w), a (h, w, 3), d (h, w, 3)); A: the albedo MEANS, not divided"""
    M, M2, a = (np.asarray(x, dtype=np.float64) for x in (M, M2, A))
    dn = np.float64(n)
    with np.errstate(all="ignore"):
        valid = np.full(M.shape[:2], int(n) >= 2) & np.isfinite(M).all(axis=2) & np.isfinite(M2).all(axis=2) & np.isfinite(a).all(axis=2)
        d = _max(a, np.float64(albedo_floor))
        I = M / d
        v = M2 / (dn - 1.0)
        u = v / (d * d)
        umax = _max(_max(_max(u[:, :, 0], u[:, :, 1]), u[:, :, 2]), 0.0)
        V = umax / dn
    return np.where(valid[:, :, None], I, M), np.where(valid, V, -1.0), valid, a, d


def denoise_albedo_mean(M, M2, n, A, iterations=ALBEDO_DEFAULTS["iterations"], sigma=ALBEDO_DEFAULTS["sigma"], eps=ALBEDO_DEFAULTS["eps"],
                        sigma_albedo=ALBEDO_DEFAULTS["sigma_albedo"], albedo_floor=ALBEDO_DEFAULTS["albedo_floor"]):
    """out, an (h, w, 3) float64 frame: C_K * d for a valid pixel, m for any other"""
    C, V, valid, a, d = prepare_albedo_mean(M, M2, n, A, albedo_floor)
    for k in range(iterations):
        C, V = albedo_helpers.iterate(C, V, valid, a, 1 << k, sigma, eps, sigma_albedo)
    with np.errstate(all="ignore"):
        return np.where(valid[:, :, None], C * d, C)


display = denoise_helpers.display


def synthetic_means(w, h, seed, n=8):
    """(M, M2, n): the fold of n made-up samples per pixel — denoise_helpers.synthetic's noisy gradients with a block of exactly zero
    variance beside another constant — then a few NaN and +-inf entries in M or M2 and, wherever the frame has room, one NEGATIVE M2
    entry and one of -0.0 (a caller may pass any M2)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.2 + 0.6 * xx / max(w - 1, 1), 0.3 + 0.5 * yy / max(h - 1, 1), 0.5 + 0.0 * xx], axis=2)
    samples = base[None] * (1.0 + 0.5 * rng.standard_normal((n, h, w, 3)))
    bx, by = w // 3, h // 3
    samples[:, by:by + max(h // 3, 1), bx:bx + max(w // 6, 1), :] = 0.25
    samples[:, by:by + max(h // 3, 1), bx + max(w // 6, 1):bx + 2 * max(w // 6, 1), :] = 0.75
    M, M2 = fold_moments(list(samples))
    if w * h >= 15:
        bad = rng.choice(w * h, size=min(8, w * h // 3), replace=False)
        for k, p in enumerate(bad[:-2]):
            (M if k % 2 else M2).reshape(-1, 3)[p, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
        M2.reshape(-1, 3)[bad[-2], :] = (-0.5, -1e-3, -2.0)   # every channel negative: max(.., 0) is what is left
        M2.reshape(-1, 3)[bad[-1], 1] = -0.0
    return M, M2, n


def synthetic_albedo_mean(w, h, seed):
    """albedo_helpers.synthetic_albedo's frame as MEANS: ramps with hard edges, exact zeros, a patch below the floor, one above 1, and
    a few NaN and +-inf entries"""
    A, n_a = albedo_helpers.synthetic_albedo(w, h, seed, n_a=4)
    with np.errstate(all="ignore"):
        return A / float(n_a)
