"""Robust frames on the CPU: the host mirror rth_robust (the kernel's own per-value body, csrc/rt_robust_shared.h) against the numpy
restatement of include/rt_amd.h "robust frames" (tests/robust_helpers.py), bit for bit — every mode, K on both sides of every boundary
between the kernel's forms, sums and means, values with ties, zeros of both signs, NaN and +inf — and the definition's stated
consequences: the trim clamp, the Gini rule's two ends on dyadic values, the invariance of `out` under the trimmed values, M2's sign."""
import numpy as np
import pytest

import robust_helpers as rh

MODE_KW = [dict(mode="mean"), dict(mode="trim", trim=1), dict(mode="trim", trim=3), dict(mode="median"), dict(mode="gini"),
           dict(mode="gini", gain=0.5), dict(mode="gini", gain=2.5)]


@pytest.mark.parametrize("K", rh.KS)
def test_the_mirror_gives_the_restatements_bits(rt, K):
    for w, h in rh.SHAPES:
        s = rh.stack(K, w, h, seed=w)
        for spp in (7, 1):                                  # sums of 7 samples per block; means
            for kw in MODE_KW:
                want, want_m2 = rh.robust(s, spp, **kw)
                got, got_m2 = rt.robust_host(s, spp, m2=True, **kw)
                assert rh.same_bits(got, want), (w, h, spp, kw, rh.differing(got, want))
                assert rh.same_bits(got_m2, want_m2), (w, h, spp, kw, rh.differing(got_m2, want_m2))
                assert rh.same_bits(rt.robust_host(s, spp, **kw), want), "without M2 the means are the same"
    # the inputs do hold what the list asks for (K >= 3: with fewer blocks there is nothing to trim and little to tie)
    if K >= 3:
        mu = rh.input_values(rh.stack(K, 65, 17, seed=65), 1)
        nans, tmax = np.isnan(mu).sum(axis=0), (K - 1) // 2
        assert (nans == 1).any() and (nans > tmax).any() and np.isinf(mu).any()
        assert ((mu == 0.0) & np.signbit(mu)).any() and ((mu == 0.0) & ~np.signbit(mu)).any()
        assert (mu == mu[0]).all(axis=0).any(), "an all-equal value"
        srt = np.sort(mu, axis=0)
        assert ((srt[1:] == srt[:-1]).any(axis=0) & ~(mu == mu[0]).all(axis=0)).any(), "exact ties among unequal blocks"


def test_a_trim_beyond_tmax_is_the_median(rt):
    for K in (1, 2, 5, 8, 17):
        s = rh.stack(K, 7, 5, seed=K)
        med = rt.robust_host(s, 3, m2=True, mode="median")
        for trim in ((K - 1) // 2, (K - 1) // 2 + 1, 40, 2 ** 31 - 1):
            got = rt.robust_host(s, 3, m2=True, mode="trim", trim=trim)
            assert rh.same_bits(got[0], med[0]) and rh.same_bits(got[1], med[1]), (K, trim)
        mean = rt.robust_host(s, 3, m2=True, mode="mean")
        got = rt.robust_host(s, 3, m2=True, mode="trim", trim=0)
        assert rh.same_bits(got[0], mean[0]) and rh.same_bits(got[1], mean[1]), K


def test_the_gini_rules_two_ends_on_dyadic_values(rt):
    """Equal blocks: W = 0, t = 0, out is the value and M2 = +0.0.  One block holding everything: W / S = K - 1 exactly, g = (K - 1) / 2
    >= tmax, t = tmax, and the median of K - 1 zeros and one value is +0.0.  Every step is exact on powers of two."""
    for K in (3, 4, 5, 8, 16, 17, 32):
        s = np.zeros((K, 2, 3, 3))
        s[:] = 0.375
        out, m2, t = rh.robust(s, 1, with_t=True)
        assert (t == 0).all()
        got, got_m2 = rt.robust_host(s, 1, m2=True)
        assert rh.same_bits(got, np.full((2, 3, 3), 0.375)) and rh.same_bits(got_m2, np.zeros((2, 3, 3)))
        s[:] = 0.0
        s[K // 3] = 64.0                                    # (the block's place in the stack is not its place in the order)
        out, m2, t = rh.robust(s, 1, with_t=True)
        assert (t == (K - 1) // 2).all()
        got, got_m2 = rt.robust_host(s, 1, m2=True)
        assert rh.same_bits(got, np.zeros((2, 3, 3))) and rh.same_bits(got_m2, np.zeros((2, 3, 3))), K
        # between the ends, at gain 1: two of eight blocks hold everything: S = 2, W = 5 + 7 = 12, g = 3 = tmax
        # and at gain 0.5: g = 1.5, t = 1 — the mean of the six central values, 1/6
    s = np.zeros((8, 1, 1, 3))
    s[2], s[5] = 1.0, 1.0
    assert (rh.robust(s, 1, with_t=True)[2] == 3).all() and rh.same_bits(rt.robust_host(s, 1), np.zeros((1, 1, 3)))
    assert (rh.robust(s, 1, gain=0.5, with_t=True)[2] == 1).all()
    assert rh.same_bits(rt.robust_host(s, 1, gain=0.5), np.full((1, 1, 3), 1.0 / 6.0))


@pytest.mark.parametrize("kw", [dict(mode="trim", trim=1), dict(mode="trim", trim=2), dict(mode="median"), dict(mode="gini"), dict(mode="gini", gain=3.0)],
                         ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_out_does_not_change_with_the_values_that_are_trimmed(rt, kw):
    """The stated invariance: the t largest values of chosen pixels times 2^20 (then +inf, then NaN), out keeps every bit — where t stays
    what it was, which under the Gini rule is asked of the restatement — and the pixels left alone keep theirs whatever happens."""
    seen = {"scaled": 0, np.inf: 0, "nan": 0}
    for K in (3, 4, 8, 9, 17, 32):
        s = rh.stack(K, 7, 5, seed=40 + K, special=False)
        s = np.abs(s)
        out, _, t = rh.robust(s, 1, with_t=True, **kw)
        flat = s.reshape(K, -1).copy()
        order = np.argsort(flat, axis=0)
        chosen = np.arange(flat.shape[1]) % 3 == 0
        for big in ("scaled", np.inf, "nan"):
            raised = flat.copy()
            for v in np.flatnonzero(chosen):
                top = order[K - t.reshape(-1)[v]:, v] if t.reshape(-1)[v] else order[:0, v]
                raised[top, v] = raised[top, v] * 2.0 ** 20 if big == "scaled" else np.float64(big)
            raised = raised.reshape(s.shape)
            out2, _, t2 = rh.robust(raised, 1, with_t=True, **kw)
            same_t = (t2 == t).reshape(-1)
            if kw["mode"] != "gini":
                assert same_t.all()
            seen[big] += int((same_t & chosen & (t.reshape(-1) >= 1)).sum())
            got = rt.robust_host(raised, 1, **kw).reshape(-1)
            base = rt.robust_host(s, 1, **kw).reshape(-1)
            assert rh.same_bits(base, out.reshape(-1))
            keep = same_t | ~chosen
            assert np.array_equal(got.view(np.uint64)[keep], base.view(np.uint64)[keep]), (K, big)
            assert np.isfinite(got[keep]).all()
        # the smallest t lowered, likewise
        lowered = flat.copy()
        for v in np.flatnonzero(chosen):
            lowered[order[:t.reshape(-1)[v], v], v] *= 2.0 ** -20
        out3, _, t3 = rh.robust(lowered.reshape(s.shape), 1, with_t=True, **kw)
        keep = (t3 == t).reshape(-1) | ~chosen
        got = rt.robust_host(lowered.reshape(s.shape), 1, **kw).reshape(-1)
        assert np.array_equal(got.view(np.uint64)[keep], out.reshape(-1).view(np.uint64)[keep]), K
    assert min(seen.values()) >= 5, (seen, "values that were trimmed, raised and trimmed as before must occur")


def test_m2_is_plus_zero_on_equal_blocks_and_never_negative(rt):
    for K in rh.KS:
        s = rh.stack(K, 7, 5, seed=3 * K)
        for kw in MODE_KW:
            _, m2 = rt.robust_host(s, 7, m2=True, **kw)
            assert not (m2 < 0.0).any() and not np.signbit(m2[m2 == 0.0]).any(), (K, kw)
            nan = np.isnan(m2)
            assert (m2.view(np.uint64)[nan] == 0x7FF8000000000000).all()
        frame = np.abs(rh.stack(1, 7, 5, seed=K, special=False)[0])
        same = np.repeat(frame[None], K, axis=0)
        for kw in MODE_KW:
            out, m2 = rt.robust_host(same, 1, m2=True, **kw)
            assert rh.same_bits(m2, np.zeros_like(frame)), (K, kw)
            assert rh.same_bits(out, frame), (K, kw)


def test_one_block_is_its_own_mean(rt):
    s = rh.stack(1, 7, 5, seed=9, special=False)
    for kw in MODE_KW:
        out, m2 = rt.robust_host(s, 4, m2=True, **kw)
        assert rh.same_bits(out, s[0] * 0.25) and rh.same_bits(m2, np.zeros_like(out)), kw
