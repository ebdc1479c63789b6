"""Shared by the frame-metrics tests (not a test module): the normative definition of include/rt_amd.h "frame metrics" in numpy, written
from the header.  Every line is one elementwise f64 operation (numpy neither contracts a * b + c nor replaces a division by a reciprocal
multiply), max(a, b) is a < b ? b : a, the reduction is the padded 256-tree, level by level, over every accumulator of an entry, and the
one logarithm comes from the oracle library's orc_log: the same fixed algorithm as the product's rt_log in a separate implementation."""
import numpy as np

INF = float("inf")
NAN = float("nan")
ERROR_FIELDS = ("count", "mse", "rmse", "rel_mse", "mae", "bias", "max_abs", "psnr")
NOISE_FIELDS = ("count", "mean_var", "noise", "max_noise")
ERROR_DEFAULTS = dict(eps=1e-2, peak=1.0)
NOISE_DEFAULTS = dict(eps=1e-2)
TEN_OVER_LN10 = 4.342944819032518
# pixel counts at which the tree changes shape: one entry, one short of a block, a block, one more, one short of two full levels, two
# full levels, and three levels
SIZES = [(1, 1), (255, 1), (256, 1), (257, 1), (257, 255), (256, 256), (257, 256)]


def bits(x):
    """the bit patterns of doubles (NaN-safe equality)"""
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same_bits(got: dict, want: dict, fields):
    g = np.array([float(got[k]) for k in fields], dtype=np.float64)
    w = np.array([float(want[k]) for k in fields], dtype=np.float64)
    return np.array_equal(bits(g), bits(w))


def means(values, spp, spp_map=None):
    """the header's "Input value": m = S * (1.0 / (double)n)"""
    values = np.asarray(values, dtype=np.float64)
    with np.errstate(all="ignore"):
        if spp_map is None:
            return values * (1.0 / np.float64(spp))
        return values * (1.0 / np.asarray(spp_map, dtype=np.float64))[..., None]


def _max(a, b):
    with np.errstate(all="ignore"):
        return np.where(a < b, b, a)


def tree(sums, maxima, counts):
    """the padded 256-tree over entries of several accumulators: `sums` and `maxima` are lists of per-pixel arrays, counts integers"""
    s = [np.asarray(a, dtype=np.float64).copy() for a in sums]
    m = [np.asarray(a, dtype=np.float64).copy() for a in maxima]
    c = np.asarray(counts, dtype=np.int64).copy()
    with np.errstate(all="ignore"):
        while True:
            pad = -len(c) % 256
            s = [np.concatenate([a, np.zeros(pad)]).reshape(-1, 256) for a in s]
            m = [np.concatenate([a, np.zeros(pad)]).reshape(-1, 256) for a in m]
            c = np.concatenate([c, np.zeros(pad, dtype=np.int64)]).reshape(-1, 256)
            stride = 128
            while stride >= 1:
                for a in s:
                    a[:, :stride] = a[:, :stride] + a[:, stride:2 * stride]
                for a in m:
                    a[:, :stride] = _max(a[:, :stride], a[:, stride:2 * stride])
                c[:, :stride] += c[:, stride:2 * stride]
                stride //= 2
            s = [a[:, 0].copy() for a in s]
            m = [a[:, 0].copy() for a in m]
            c = c[:, 0].copy()
            if len(c) == 1:
                return [float(a[0]) for a in s], [float(a[0]) for a in m], int(c[0])


def _three(t):
    with np.errstate(all="ignore"):
        return (t[:, 0] + t[:, 1]) + t[:, 2]


def frame_error(values, spp, ref, ref_spp, *, spp_map=None, eps=ERROR_DEFAULTS["eps"], peak=ERROR_DEFAULTS["peak"]):
    import oracle_lib
    m = means(values, spp, spp_map).reshape(-1, 3)
    r = means(ref, ref_spp).reshape(-1, 3)
    counts = np.isfinite(m).all(axis=1) & np.isfinite(r).all(axis=1)
    with np.errstate(all="ignore"):
        d = m - r
        sq = d * d
        ab = np.abs(d)
        den = (r * r) + np.float64(eps)
        rel = sq / den
        terms = [_three(sq), _three(rel), _three(ab), _three(d)]
        mx = _max(_max(ab[:, 0], ab[:, 1]), ab[:, 2])
    terms = [np.where(counts, t, 0.0) for t in terms]
    mx = np.where(counts, mx, 0.0)
    (T_sq, T_rel, T_ab, T_d), (T_max,), count = tree(terms, [mx], counts)
    if count == 0:
        return dict.fromkeys(ERROR_FIELDS, 0.0) | {"count": 0}
    with np.errstate(all="ignore"):
        N = np.float64(3 * count)
        mse = np.float64(T_sq) / N
        psnr = INF if mse == 0.0 else float(np.float64(TEN_OVER_LN10) * np.float64(
            oracle_lib.lib().orc_log(float((np.float64(peak) * np.float64(peak)) / mse))))
        return dict(count=count, mse=float(mse), rmse=float(np.sqrt(mse)), rel_mse=float(np.float64(T_rel) / N), mae=float(np.float64(T_ab) / N),
                    bias=float(np.float64(T_d) / N), max_abs=float(T_max), psnr=psnr)


def channel_variance(a, b, n, means_form):
    """(h * w, 3) var_c and the (h * w,) counting mask; n: an int or a per-pixel integer array"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    n = np.broadcast_to(np.asarray(n, dtype=np.int64).reshape(-1), (len(a),))
    dn = n.astype(np.float64)[:, None]
    counts = (n >= 2) & np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
    with np.errstate(all="ignore"):
        if means_form:
            v = b / (dn - 1.0)
        else:
            m = a / dn
            v = (b - a * m) / (dn - 1.0)
        v = np.where(0.0 > v, 0.0, v)
        var = v / dn
    return var, counts


def frame_noise(a, b, n, *, form="sums", spp_map=None, eps=NOISE_DEFAULTS["eps"]):
    means_form = form == "means"
    per_pixel = n if spp_map is None else np.asarray(spp_map)
    var, counts = channel_variance(a, b, per_pixel, means_form)
    a = np.asarray(a, dtype=np.float64)
    mean = (a if means_form else means(a, n, spp_map)).reshape(-1, 3)
    with np.errstate(all="ignore"):
        rel = var / ((mean * mean) + np.float64(eps))
        V, R = _three(var), _three(rel)
        mx = _max(_max(rel[:, 0], rel[:, 1]), rel[:, 2])
    (T_v, T_r), (T_max,), count = tree([np.where(counts, V, 0.0), np.where(counts, R, 0.0)], [np.where(counts, mx, 0.0)], counts)
    if count == 0:
        return dict(count=0, mean_var=0.0, noise=INF, max_noise=INF)
    with np.errstate(all="ignore"):
        N = np.float64(3 * count)
        return dict(count=count, mean_var=float(np.float64(T_v) / N), noise=float(np.sqrt(np.float64(T_r) / N)), max_noise=float(np.sqrt(np.float64(T_max))))


def frame_pair(w, h, seed=7):
    """(frame, reference) of means, (h, w, 3) each, with a fixed seed: radiances of mixed magnitude around a reference, and planted values
    above 1, exact zeros, negative values, pixels equal to the reference (pixel 0 always: a 1 x 1 frame has mse == 0) and, from 8 pixels
    on, a NaN and both infinities in frame or reference"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    n = w * h
    ref = 10.0 ** rng.uniform(-3.0, 1.5, size=(n, 3))
    frame = ref * (1.0 + rng.normal(0.0, 0.2, size=(n, 3)))
    frame[0] = ref[0]                       # equal to the reference
    if n >= 8:
        frame[1] = (0.0, 0.0, 0.0)          # exact zeros
        ref[2] = (0.0, 0.5, 0.0)
        frame[3] = (-0.25, 2.5, -1e-3)      # negative values, a value above 1
        frame[4, 1] = NAN                   # does not count
        ref[5, 2] = INF                     # does not count
        frame[6, 0] = -INF                  # does not count
        frame[n - 1] = ref[n - 1]           # equal, in the last (ragged) block
        ref[n // 2] = (40.0, 17.5, 3.0)     # well above 1
    return frame.reshape(h, w, 3), ref.reshape(h, w, 3)


def moments(w, h, n, seed=11):
    """(S, Q) sums and sums of squares of n samples per pixel, (h, w, 3) each, with planted zero variance, a negative v_c from rounding, and
    (from 8 pixels on) a non-finite moment"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    p = w * h
    mean = 10.0 ** rng.uniform(-2.0, 1.0, size=(p, 3))
    spread = mean * rng.uniform(0.0, 1.5, size=(p, 3))
    S = mean * n
    Q = (mean * mean + spread * spread) * n
    S[0] = (0.3 * n, 0.3 * n, 0.3 * n)
    Q[0] = (0.3 * 0.3 * n,) * 3             # zero variance up to rounding: v_c may come out negative and is clamped
    if p >= 8:
        S[1] = 0.0
        Q[1] = 0.0
        Q[3, 0] = NAN
        S[4, 2] = INF
    return S.reshape(h, w, 3), Q.reshape(h, w, 3)


def mean_moments(w, h, n, seed=13):
    """(mean, M2) of the means form from the same generator"""
    S, Q = moments(w, h, n, seed)
    with np.errstate(all="ignore"):
        mean = S / n
        m2 = np.where(np.isfinite(Q), np.maximum(Q - S * mean, 0.0), Q)
    return mean, m2


def spp_map_for(w, h):
    """an (h, w) int32 map of 1..4 samples: the entries that are 1 do not count in the noise call"""
    return (1 + (np.arange(w * h, dtype=np.int64) * 5) % 4).astype(np.int32).reshape(h, w)
