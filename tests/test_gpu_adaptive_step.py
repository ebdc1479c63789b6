"""One convergence step of adaptive sampling on chosen inputs (rt_debug_adaptive_step: the render's own three kernels and scratch
layout, nothing rendered), against a numpy reference: the rule as adaptive_helpers.replay has it, the compaction as
`survivors = list[keep]` in list order.  Every array the kernels must not write carries a sentinel.

Compaction: lists of 64 entries to 4 M (1, 2, 3 and 17 trips of the scan kernel's loop over 1024 blocks), every keep pattern, pads,
shuffled lists, the last schedule point.  The verdicts there come from S = Q = 0 (converges under any threshold) and a NaN in S (never
does), not from the arithmetic under test.

The rule: random (S, Q) around the threshold at several (n, rel, abs), and constructed families — exact ties and their
neighbours, products that a fused multiply-add would round differently, negative and zero variance, n = 2 and 2^24, subnormal and
non-finite sums, a tolerance whose square overflows.  The hook takes ONE (n, rel, abs) per call, so a family is a list of groups, each
a call; the builders are plain functions and tests/test_adaptive_abi.py proves on the CPU that every family holds both verdicts
(and, for the contraction family, at least 10 000 cases whose fused verdict differs).

Added GPU time, measured on an MI355X: about 5 s for the file (the 4 M-entry lists: 1.3 s of it)."""
from fractions import Fraction

import numpy as np
import pytest

from adaptive_helpers import PAD, pad64, replay

pytestmark = pytest.mark.gpu

SPP_SENTINEL = -77
LIST_SENTINEL = 0xABCD1234  # (no pixel index: the frames here have fewer than 2^27 pixels)
CHUNK = 1024 * 256          # list entries per trip of the scan kernel's loop
SIZES = [64, 192, 256, 320, CHUNK - 64, CHUNK, CHUNK + 64, 2 * CHUNK + 64 * 5, 960_000, 16 * CHUNK + 64 * 3]


def reference_step(pixels, S, Q, n, rel, abs_, last=False):
    """(survivors in list order, the pixels that leave)"""
    n_pixels = S.shape[0]
    listed = pixels < n_pixels
    e = pixels[listed].astype(np.int64)
    with np.errstate(all="ignore"):
        done = np.ones(e.size, dtype=bool) if last else (replay(S[e], Q[e], n, rel, abs_) if n >= 2 else np.zeros(e.size, dtype=bool))
    keep = np.zeros(pixels.size, dtype=bool)
    keep[listed] = ~done
    return pixels[keep], e[done]


def check_step(rt, pixels, S, Q, n, rel, abs_, last=False, what=""):
    pixels = np.ascontiguousarray(pixels, dtype=np.uint32)
    n_pixels = S.shape[0]
    survivors, leavers = reference_step(pixels, S, Q, n, rel, abs_, last)
    spp0 = np.full(n_pixels, SPP_SENTINEL, dtype=np.int32)
    out0 = np.full(pixels.size, LIST_SENTINEL, dtype=np.uint32)
    count, list_out, spp = rt.debug_adaptive_step(pixels, S, Q, n, rel, abs_, last=last, spp=spp0, list_out=out0)
    assert count == survivors.size, f"{what}: {count} survivors, the reference has {survivors.size}"
    assert np.array_equal(list_out[:count], survivors), f"{what}: the survivors differ (first at {int(np.flatnonzero(list_out[:count] != survivors)[0])})"
    assert (list_out[count:pad64(count)] == PAD).all(), f"{what}: the tail up to a multiple of 64 is not padding"
    assert (list_out[pad64(count):] == LIST_SENTINEL).all(), f"{what}: list_out was written beyond the padded survivors"
    want_spp = spp0.copy()
    want_spp[leavers] = n
    assert np.array_equal(spp, want_spp), f"{what}: spp differs at {int((spp != want_spp).sum())} pixels"
    return count


# ---- compaction ------------------------------------------------------------------------------------------------------------------------
def keep_patterns(size, g):
    """name -> bool per list position: who survives"""
    pos = np.arange(size)
    waves, blocks = size // 64, (size + 255) // 256
    one = lambda at: np.isin(pos, at)
    block = blocks - 1  # (a partial one where the size is no multiple of 256; beyond the scan's first trip where there are several)
    return {
        "nobody": np.zeros(size, dtype=bool),
        "everybody": np.ones(size, dtype=bool),
        "first": one([0]),
        "last": one([size - 1]),
        "one_per_wave": one(np.arange(waves) * 64 + (np.arange(waves) * 7) % 64),
        "one_per_block": one(np.minimum(np.arange(blocks) * 256 + (np.arange(blocks) * 37) % 256, size - 1)),
        "one_block": (pos >> 8) == block,
        "middle_block": (pos >> 8) == blocks // 2,
        "alternating": (pos & 1) == 1,
        "random_1_64": g.random(size) < 1 / 64,
        "random_1_2": g.random(size) < 1 / 2,
        "random_63_64": g.random(size) < 63 / 64,
    }


def build_list(size, n_pixels, g, pads, shuffled):
    """A list of `size` distinct pixels of n_pixels (some stay unlisted); pads: some entries scattered, wave 1 and a whole block."""
    pixels = g.permutation(n_pixels)[:size].astype(np.uint32) if shuffled else np.arange(size, dtype=np.uint32)
    if pads:
        pixels[g.random(size) < 0.03] = PAD
        if size >= 128:
            pixels[64:128] = PAD
        if size >= 1024:
            b = (size // 256) // 2 + 1
            pixels[b * 256:(b + 1) * 256] = PAD
    return pixels


def compaction_case(size, name, keep, g, pads=False, shuffled=False):
    n_pixels = size + 100
    pixels = build_list(size, n_pixels, g, pads, shuffled)
    S = np.zeros((n_pixels, 3))
    Q = np.zeros((n_pixels, 3))
    survivors = pixels[keep & (pixels != PAD)]
    S[survivors, g.integers(0, 3, survivors.size)] = np.nan
    return pixels, S, Q


LARGE_PATTERNS = {  # a handful per large size; every pattern at some size of more than one scan trip
    CHUNK - 64: ["everybody", "last", "random_1_2"],
    CHUNK: ["nobody", "one_per_block", "alternating"],
    CHUNK + 64: ["first", "one_block", "random_63_64", "last"],
    2 * CHUNK + 64 * 5: ["one_per_wave", "random_1_64", "everybody", "one_block", "middle_block"],
    960_000: ["random_1_2", "one_per_block", "alternating", "last"],
    16 * CHUNK + 64 * 3: ["random_1_2", "last", "one_block"],
}


@pytest.mark.parametrize("size", SIZES)
def test_compaction_keeps_the_survivors_in_list_order(rt, gpu, size):
    g = np.random.default_rng(size)
    patterns = keep_patterns(size, g)
    names = LARGE_PATTERNS.get(size, list(patterns))
    for k, name in enumerate(names):
        # plain, then with pads, then shuffled with pads: each pattern once, the variants in turn (small sizes: all three)
        variants = [(False, False), (True, False), (True, True)] if size <= 320 else [[(False, False), (True, False), (True, True)][k % 3]]
        for pads, shuffled in variants:
            pixels, S, Q = compaction_case(size, name, patterns[name], g, pads, shuffled)
            count = check_step(rt, pixels, S, Q, 4, 0.0, 1.0, what=f"{size} {name} pads={pads} shuffled={shuffled}")
            assert count == int((patterns[name] & (pixels != PAD)).sum())


@pytest.mark.parametrize("size", [64, 320, CHUNK + 64, 16 * CHUNK + 64 * 3])
def test_the_last_schedule_point_empties_the_list(rt, gpu, size):
    g = np.random.default_rng(size + 1)
    pixels, S, Q = compaction_case(size, "random_1_2", g.random(size) < 0.5, g, pads=True, shuffled=size != 320)
    assert check_step(rt, pixels, S, Q, 9, 0.0, 0.0, last=True, what=f"{size} last") == 0


def test_a_list_that_is_no_multiple_of_64_is_refused(rt, gpu):
    S = np.zeros((100, 3))
    for bad in (1, 63, 65, 100):
        with pytest.raises(rt.RtError, match="multiple of 64"):
            rt.debug_adaptive_step(np.arange(bad, dtype=np.uint32), S, S, 4, 0.0, 1.0)


# ---- the rule: groups of (name, S, Q, n, rel, abs), one hook call each --------------------------------------------------------------------
def verdicts(S, Q, n, rel, abs_):
    with np.errstate(all="ignore"):
        return replay(S, Q, n, rel, abs_)


def random_value_groups(count=CHUNK, seed=11):
    """(S, Q) with e2 spread around tol^2 by a factor e either way, the maximum in a random channel."""
    g = np.random.default_rng(seed)
    groups = []
    for n, rel, abs_ in [(2, 0.05, 1e-3), (3, 0.0, 0.02), (17, 0.1, 0.0), (64, 0.02, 1e-3), (1000, 0.3, 1e-6), (1 << 24, 0.01, 1e-4)]:
        mu = g.random((count, 3)) * 2.0
        S = mu * n
        tol = rel * mu.mean(axis=1) + abs_
        e2 = tol * tol * np.exp(g.uniform(-1.0, 1.0, count))
        var = np.outer(e2 * n, np.ones(3)) * g.random((count, 3))
        var[np.arange(count), g.integers(0, 3, count)] = e2 * n
        Q = S * S / n + var * (n - 1)
        groups.append((f"random n={n}", S, Q, n, rel, abs_))
    return groups


def tie_groups():
    """n = 4, S = (4, 4, 4), rel = abs = 1/4: m = 1, tol^2 = 1/4, and Q = 7 in the largest channel gives e2 = 1/4 exactly; n = 2,
    S = (2, 2, 2): Q = 5/2 does.  Each with its two neighbours, in every channel, scaled by powers of two (S, abs by 2^j, Q by 4^j)."""
    groups = []
    for n, q_tie, q_low in ((4, 7.0, 5.0), (2, 2.5, 2.25)):
        for j in (-300, -40, -1, 0, 3, 52, 200):
            s, s2 = 2.0 ** j, 4.0 ** j
            S, Q = [], []
            for c in range(3):
                for q in (q_tie, np.nextafter(q_tie, np.inf), np.nextafter(q_tie, 0.0)):
                    row = [q_low * s2] * 3
                    row[c] = q * s2
                    S.append([n * s] * 3)
                    Q.append(row)
            groups.append((f"tie n={n} 2^{j}", np.array(S), np.array(Q), n, 0.25, 0.25 * s))
    return groups


def _fused_e2(S, m, Q, n):
    """e2 of one channel if Q - S * m were rounded once (a fused multiply-add), the divisions as the rule has them"""
    d = float(Fraction(Q) - Fraction(S) * Fraction(m))
    return np.float64(d) / np.float64(n - 1) / np.float64(n)


def contraction_groups(per_group=6144, seed=5):
    """Q = fl(S * m) + k ulps, so that Q - S * m cancels to a few ulps: rounded twice it is exactly k ulps, rounded once (fused)
    k + d ulps, d the product's own rounding error in (-1/2, 1/2).  With rel = 0 and abs^2 a quarter of an ulp above (below) k ulps'
    worth of e2, the cases with d beyond that quarter get the other verdict from a fused evaluation.  The other channels hold
    S = Q = 0.  Returns the groups and, per group, the mask of the cases whose fused verdict differs (exact rational arithmetic)."""
    g = np.random.default_rng(seed)
    groups, sensitive = [], []
    for n, k, side, exp in [(2, 1, +1, 0), (3, 2, -1, 3), (7, 1, -1, -9), (10, 3, +1, 6), (31, 2, +1, 0), (100, 1, +1, -2),
                            (199, 4, -1, 10), (64, 2, -1, 1), (5, 1, +1, 30), (13, 3, -1, -30), (150, 2, +1, 4), (2, 5, -1, 0)]:
        lo = 2.0 ** exp  # S^2 / n in [lo, 2 lo): one binade, one ulp
        s = np.sqrt(n * lo * (1.02 + 0.95 * g.random(per_group)))
        m = s / n
        P = s * m
        u = np.spacing(lo)
        q = P + k * u
        abs_ = float(np.sqrt((k + 0.25 * side) * u / (n * (n - 1.0))))
        c = g.integers(0, 3, per_group)
        S = np.zeros((per_group, 3))
        Q = np.zeros((per_group, 3))
        S[np.arange(per_group), c] = s
        Q[np.arange(per_group), c] = q
        two = verdicts(S, Q, n, 0.0, abs_)
        tol2 = np.float64(abs_) * np.float64(abs_)
        # (the zero channels' variance is 0, below the positive one here, so the fused e2 is this channel's)
        fused = np.array([max(_fused_e2(s[i], m[i], q[i], n), 0.0) <= tol2 for i in range(per_group)])
        groups.append((f"contraction n={n} k={k} side={side}", S, Q, n, 0.0, abs_))
        sensitive.append(fused != two)
    return groups, sensitive


def cancellation_groups(count=4096, seed=9):
    """Q from 3 ulps below fl(S * m) to 3 above, rel = abs = 0: only e2 <= 0 converges — a negative variance does, a positive does not."""
    g = np.random.default_rng(seed)
    groups = []
    for n in (2, 5, 1000):
        S = g.uniform(0.1, 50.0, (count, 3))
        P = S * (S / n)
        k = g.integers(-3, 4, (count, 3))
        Q = P + k * np.spacing(P)
        groups.append((f"cancellation n={n}", S, Q, n, 0.0, 0.0))
        groups.append((f"cancellation n={n} abs", S, Q, n, 0.0, float(np.sqrt(np.spacing(P).mean() / n / n))))
    return groups


def edge_groups():
    inf, nan, tiny = np.inf, np.nan, 5e-324
    groups = []
    # a non-finite value in any one channel of S or of Q never converges, whatever the tolerance; the finite rows beside them do
    S, Q = [[1.0, 2.0, 3.0]], [[1.0, 2.0, 3.0]]
    for bad in (inf, -inf, nan):
        for c in range(3):
            for which in (0, 1):
                s, q = [3.0, 3.0, 3.0], [3.0, 3.0, 3.0]
                (s, q)[which][c] = bad
                S.append(s)
                Q.append(q)
    groups.append(("non-finite", np.array(S), np.array(Q), 3, 1.0, 1e300))
    # zero sums, zero thresholds: e2 = 0 <= 0 converges; any positive variance does not
    S = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [2.0, 2.0, 2.0], [2.0, 2.0, 2.0], [-0.0, 0.0, -0.0]])
    Q = np.array([[0.0, 0.0, 0.0], [0.0, tiny * 4, 0.0], [2.0, 2.0, 2.0], [2.0, np.nextafter(2.0, 3.0), 2.0], [0.0, -0.0, 0.0]])
    for n in (2, 3):
        groups.append((f"zero n={n}", S, Q if n == 2 else Q * np.array([1.0, 1.0, 2.0 / 3.0, 2.0 / 3.0, 1.0])[:, None], n, 0.0, 0.0))
    # subnormal sums: the means and the products underflow, rel * L stays subnormal and its square is 0
    j = np.arange(1, 41, dtype=np.float64)
    S = np.outer(j * tiny, [1.0, 2.0, 3.0])
    Q = np.outer(np.where(np.arange(40) % 3 == 0, 0.0, (np.arange(40) % 5) * tiny), [1.0, 1.0, 1.0])
    groups.append(("subnormal n=3", S, Q, 3, 1.0, 0.0))
    groups.append(("subnormal n=2", S, Q, 2, 0.5, tiny))
    # tol^2 overflows to +inf: every finite variance converges, also one whose product overflowed to -inf; a NaN variance cannot
    # arise from finite sums, and non-finite sums still never converge
    S = np.array([[1e3, 1e3, 1e3], [1e200, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, inf, 1.0], [-1e200, 1e200, 0.0]])
    Q = np.array([[1e300, 1e308, 1.0], [1.0, 1.0, 1.0], [1.7e308, 1.7e308, 1.7e308], [1.0, 1.0, 1.0], [1e308, 0.0, 1e-300]])
    groups.append(("tol^2 overflows", S, Q, 2, 0.0, 1e200))
    groups.append(("huge variance", S, Q, 2, 0.0, 1e100))
    # n = 2^24: the largest count the schedule's int32 arithmetic is documented for
    n = 1 << 24
    g = np.random.default_rng(3)
    S = g.uniform(0.0, 3.0, (512, 3)) * n
    Q = S * S / n + g.uniform(0.0, 2.0, (512, 3)) * 1e-6 * n * (n - 1.0)
    groups.append(("n = 2^24", S, Q, n, 0.0, 1e-3))
    return groups


def run_groups(rt, groups, shuffle_seed=1):
    """Each group through the hook, its pixels listed in a shuffled order with pads between them; returns the device's verdicts."""
    g = np.random.default_rng(shuffle_seed)
    out = []
    for name, S, Q, n, rel, abs_ in groups:
        count = S.shape[0]
        pixels = np.full(pad64(count + 64), PAD, dtype=np.uint32)
        pixels[g.permutation(pixels.size)[:count]] = g.permutation(count).astype(np.uint32)
        check_step(rt, pixels, S, Q, n, rel, abs_, what=name)
        _, _, spp = rt.debug_adaptive_step(pixels, S, Q, n, rel, abs_)
        out.append(spp == n)
    return out


def test_random_values_get_the_references_verdict_across_the_scans_chunk(rt, gpu):
    groups = random_value_groups()
    assert pad64(groups[0][1].shape[0] + 64) >= CHUNK + 64
    for (name, S, Q, n, rel, abs_), got in zip(groups, run_groups(rt, groups)):
        want = verdicts(S, Q, n, rel, abs_)
        assert 0.2 < want.mean() < 0.8, (name, want.mean())
        assert np.array_equal(got, want), name


@pytest.mark.parametrize("family", [tie_groups, cancellation_groups, edge_groups])
def test_constructed_families_get_the_references_verdict(rt, gpu, family):
    groups = family()
    for (name, S, Q, n, rel, abs_), got in zip(groups, run_groups(rt, groups)):
        assert np.array_equal(got, verdicts(S, Q, n, rel, abs_)), name


def test_products_a_fused_multiply_add_would_round_differently_get_the_two_rounding_verdict(rt, gpu):
    groups, sensitive = contraction_groups()
    assert sum(int(s.sum()) for s in sensitive) >= 10_000
    for (name, S, Q, n, rel, abs_), sens, got in zip(groups, sensitive, run_groups(rt, groups)):
        want = verdicts(S, Q, n, rel, abs_)
        wrong = got != want
        assert not wrong.any(), f"{name}: {int(wrong.sum())} verdicts differ, {int((wrong & sens).sum())} of them where a fused product would"
