"""The definition of include/rt_amd.h "robust frames" restated in numpy from the header's text, one rounded f64 operation per step
(numpy does not contract a multiplication and an addition of two separate ufunc calls), and the inputs the robust tests share."""
import numpy as np

MEAN, TRIM, MEDIAN, GINI = 0, 1, 2, 3
MODES = {"mean": MEAN, "trim": TRIM, "median": MEDIAN, "gini": GINI}
DEFAULTS = dict(mode=GINI, trim=1, gain=1.0)
MAX_BLOCKS = 32
THE_NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
# even and odd K, both sides of every boundary between the kernel's forms (4, 8, 16, 32 slots), and the maximum
KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)
SHAPES = [(1, 1), (7, 5), (65, 17)]
GPU_SHAPES = SHAPES + [(130, 70),   # no multiple of any workgroup size
                       (256, 8)]    # 3 w h = 6144 values: 24 workgroups of 256 exactly


def _the_nan(x):
    return np.where(np.isnan(x), THE_NAN, x)


def input_values(stack, spp):
    """mu_k = S_k * (1.0 / (double)spp), every NaN replaced by THE NaN; (K, n)"""
    stack = np.asarray(stack, dtype=np.float64)
    with np.errstate(all="ignore"):
        return _the_nan(stack.reshape(stack.shape[0], -1) * (np.float64(1.0) / np.float64(spp)))


def trim_counts(mu_sorted, mode=GINI, trim=1, gain=1.0):
    """t per value, from the values in order"""
    K, n = mu_sorted.shape
    tmax = (K - 1) // 2
    if mode == MEAN:
        return np.zeros(n, dtype=np.int64)
    if mode == TRIM:
        return np.full(n, min(int(trim), tmax), dtype=np.int64)
    if mode == MEDIAN:
        return np.full(n, tmax, dtype=np.int64)
    assert mode == GINI
    with np.errstate(all="ignore"):
        S, W = np.zeros(n), np.zeros(n)
        for i in range(K):
            S = S + mu_sorted[i]
            W = W + (np.float64(2 * i - K + 1) * mu_sorted[i])
        g = (np.float64(gain) * (W / S)) * np.float64(0.5)
        below = g < np.float64(tmax)
        t = np.where(below, np.trunc(np.where(below, g, 0.0)), tmax).astype(np.int64)
        t = np.where((S > 0.0) & (W > 0.0), t, 0)
    return np.where(np.isfinite(mu_sorted).all(axis=0), t, tmax)


def robust(stack, spp, *, mode=GINI, trim=1, gain=1.0, with_t=False):
    """(out, M2[, t]) of a (K, h, w, 3) stack, each (h, w, 3)"""
    mode = MODES.get(mode, mode)
    stack = np.asarray(stack, dtype=np.float64)
    K = stack.shape[0]
    mu = np.sort(input_values(stack, spp), axis=0)    # ascending; numpy puts NaN behind +inf and holds -0.0 == +0.0
    t = trim_counts(mu, mode, trim, gain)
    last = K - 1 - t
    with np.errstate(all="ignore"):
        acc = np.zeros(mu.shape[1])
        for i in range(K):
            acc = np.where((i >= t) & (i <= last), acc + mu[i], acc)
        lo, hi = np.take_along_axis(mu, t[None], 0)[0], np.take_along_axis(mu, last[None], 0)[0]
        out = np.where(lo == hi, lo + 0.0, _the_nan(acc / (K - 2 * t).astype(np.float64)))
        q = np.zeros(mu.shape[1])
        for i in range(K):
            w = np.where(i < t, lo, np.where(i > last, hi, mu[i]))
            d = w - out
            q = q + (d * d)
        q = _the_nan(q)
    shape = stack.shape[1:]
    res = (out.reshape(shape), q.reshape(shape))
    return res + (t.reshape(shape),) if with_t else res


def stack(K, w, h, seed=0, special=True):
    """a (K, h, w, 3) stack of block SUMS as a render gives them — positive, a common level per value with block-to-block noise, and a
    firefly (x 50 .. 5000) in one block of every sixth value — and, `special`, per value of chosen pixels: exact ties, -0.0 beside
    +0.0, a NaN in one block, +inf in one block, NaNs in more than tmax blocks, and an all-equal pixel; seeded"""
    rng = np.random.default_rng(3000 + 97 * K + seed)
    n = w * h * 3
    level = 10.0 ** rng.uniform(-3.0, 2.0, size=n)
    s = level[None] * rng.lognormal(0.0, 0.4, size=(K, n))
    hot = np.flatnonzero(rng.random(n) < 1.0 / 6.0)
    s[rng.integers(0, K, size=hot.size), hot] *= 10.0 ** rng.uniform(1.7, 3.7, size=hot.size)
    s[:, rng.random(n) < 0.05] *= -1.0                  # (a stack need not be radiance: some values negative in every block)
    if special:
        tmax = (K - 1) // 2
        picks = rng.permutation(n)

        def some(j):                                    # every seventh value from j on: the specials never share a value
            return picks[j::7][:max(1, n // 14)]
        v = some(0)                                     # exact ties: half of the blocks share one value
        s[: (K + 1) // 2, v] = s[0, v]
        v = some(1)                                     # zeros of both signs, alternating
        s[:, v] = np.where(np.arange(K)[:, None] % 2 == 0, -0.0, 0.0)
        v = some(2)                                     # -0.0 and +0.0 beside real values
        s[0, v], s[K - 1, v] = -0.0, 0.0
        v = some(3)
        s[rng.integers(0, K, size=v.size), v] = np.nan
        v = some(4)
        s[rng.integers(0, K, size=v.size), v] = np.inf
        v = some(5)                                     # NaNs in more than tmax blocks
        s[: tmax + 1, v] = np.nan
        v = some(6)                                     # all blocks equal
        s[:, v] = s[0, v]
    return np.ascontiguousarray(s.reshape(K, h, w, 3))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).sum())
