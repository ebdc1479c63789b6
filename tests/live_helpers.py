"""Shared by the live-refinement tests (not a test module): the running-mean recurrence of include/rt_amd.h "live refinement" in numpy,
and the expected frames built from the CPU oracle's single-sample renders."""
import numpy as np


def fold(colours, mean=None, first=0):
    """m = m + (c_s - m) / (s + 1) for s = first, first + 1, ...: three elementwise f64 operations per sample, each rounded on its own
    (numpy neither contracts nor replaces the division by a reciprocal multiply).  `mean`: the value after `first` samples (+0.0 if None)."""
    m = np.zeros_like(np.asarray(colours[0], dtype=np.float64)) if mean is None else np.array(mean, dtype=np.float64)
    for k, c in enumerate(colours):
        d = np.asarray(c, dtype=np.float64) - m
        q = d / np.float64(first + k + 1)
        m = m + q
    return m


def fold_by_reciprocal(colours):
    """the recurrence with (c - m) * (1 / n) in place of the division: what the library must NOT compute"""
    m = np.zeros_like(np.asarray(colours[0], dtype=np.float64))
    for k, c in enumerate(colours):
        d = np.asarray(c, dtype=np.float64) - m
        q = d * (np.float64(1.0) / np.float64(k + 1))
        m = m + q
    return m


def oracle_samples(rt, oracle, hs, n, seed):
    """[colour of sample s for s in 0 .. n - 1], each a frame of 3 w h doubles: orc_render over [s, s + 1) is 0 + c_s"""
    out = []
    for s in range(n):
        c = oracle.render(hs, rt.render_params(seed=seed, sample_begin=s, sample_end=s + 1))
        c.setflags(write=False)
        out.append(c)
    return out
