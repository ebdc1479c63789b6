"""The host mirror of guided upsampling (rth_upsample; no GPU) against the numpy restatement of include/rt_amd.h "guided upsampling" in
tests/upsample_helpers.py, bit for bit: every listed size at every factor with every guide set, non-finite pixels in the low frame and
in the guides, the three consequences the header states, inputs on which another accumulation order gives other bits, and the synthetic
step on which the edge guide must beat the plain tent."""
import numpy as np
import pytest

import upsample_helpers as uh


@pytest.fixture(scope="module")
def cases():
    """per (w, h, F): the shared inputs, with non-finite values, never written"""
    out = {}
    for w, h in uh.HOST_SHAPES:
        for F in uh.FACTORS:
            low, spp, alb, edge = uh.inputs(w, h, F, seed=w + h, special=True)
            for a in (low, alb[0], edge[0]):
                a.setflags(write=False)
            out[(w, h, F)] = (low, spp, alb, edge)
    return out


@pytest.mark.parametrize("F", uh.FACTORS)
@pytest.mark.parametrize("w,h", uh.HOST_SHAPES, ids=lambda v: str(v))
def test_the_mirror_gives_the_restated_bits_and_the_display_bytes(rt, cases, w, h, F):
    low, spp, alb, edge = cases[(w, h, F)]
    if w * h > 4:
        assert not np.isfinite(low).all() and not np.isfinite(alb[0]).all() and not np.isfinite(edge[0]).all()
    kw = dict(factor=F, sigma_edge=0.4, sigma_albedo=0.6, albedo_floor=2e-3)
    results = {}
    for kind in uh.GUIDE_SETS:
        g = uh.guides_for(kind, alb, edge)
        want = uh.upsample(low, spp, (w, h), **g, **kw)
        got, rgba = rt.upsample_host(low, spp, (w, h), rgba8=True, **g, **kw)
        assert got.shape == (h, w, 3) and rgba.shape == (h, w, 4)
        assert uh.same_bits(got, want), (kind, int((got.view(np.uint64) != want.view(np.uint64)).sum()))
        assert np.array_equal(rgba, rt.tonemap_host(got, 1, rgba8=True)[1]), kind    # (the clamp: the bytes of rt_resolve_rgba8_device)
        assert uh.same_bits(rt.upsample_host(low, spp, (w, h), **g, **kw), got), "without the bytes"
        results[kind] = got
    if w * h >= 91:   # (the small frames' few low pixels may all be invalid)
        assert not uh.same_bits(results["none"], results["edge"]) and not uh.same_bits(results["albedo"], results["both"]), "the guides must bite"
    if F == 2:
        assert uh.same_bits(rt.upsample_host(low, spp, (w, h), **uh.guides_for("both", alb, edge)),
                            uh.upsample(low, spp, (w, h), **uh.guides_for("both", alb, edge), **uh.DEFAULTS))   # the defaults are the header's


def test_the_input_tells_accumulation_orders_apart(rt):
    w, h = 13, 7
    for F in uh.FACTORS:
        low, spp, alb, edge = uh.inputs(w, h, F, seed=20)
        for kind in ("none", "both"):
            g = uh.guides_for(kind, alb, edge)
            forward, backward = uh.upsample(low, spp, (w, h), factor=F, **g), uh.upsample(low, spp, (w, h), factor=F, reverse=True, **g)
            assert (forward != backward).any(), "the input must tell ((w1 R1 + w2 R2) + w3 R3) + ... from the sum taken from the other end"
            assert np.allclose(forward, backward, rtol=1e-9, atol=1e-9 * float(np.abs(forward).max()))
            got = rt.upsample_host(low, spp, (w, h), factor=F, **g)
            assert uh.same_bits(got, forward) and not uh.same_bits(got, backward), (F, kind)


def test_a_non_finite_low_pixel_stays_in_its_own_block(rt):
    w, h = 17, 11
    for F in uh.FACTORS:
        low, spp, alb, edge = uh.inputs(w, h, F, seed=31)
        lh, lw = low.shape[:2]
        bad = [(1, 2, 0, np.nan), (lh - 1, lw - 1, 1, np.inf), (2, 0, 2, -np.inf)]
        dirty = low.copy()
        for J, I, c, value in bad:
            dirty[J, I, c] = value
        own = np.zeros((h, w), dtype=bool)
        for J, I, _, _ in bad:
            own[F * J:F * J + F, F * I:F * I + F] = True
        for kind in uh.GUIDE_SETS:
            g = uh.guides_for(kind, alb, edge)
            got = rt.upsample_host(dirty, spp, (w, h), factor=F, **g)
            assert uh.same_bits(got, uh.upsample(dirty, spp, (w, h), factor=F, **g))
            assert np.isfinite(got[~own]).all(), (F, kind)
            # ... and is no tap: every other pixel gets what it gets when the low pixel is simply not there — which no finite value in its
            # place gives, so compare with the restatement's frame of a low frame whose bad pixels are marked invalid by another NaN
            other = dirty.copy()
            for J, I, c, _ in bad:
                other[J, I] = np.nan
            assert uh.same_bits(got[~own], rt.upsample_host(other, spp, (w, h), factor=F, **g)[~own])


def test_a_non_finite_guide_pixel_stays_in_its_own_block(rt):
    w, h = 17, 11
    for F in uh.FACTORS:
        low, spp, (A, n_a), (E, n_e) = uh.inputs(w, h, F, seed=37)
        bad = [(3, 5, 0, np.nan), (h - 1, w - 1, 1, np.inf), (6, 0, 2, -np.inf)]
        own = np.zeros((h, w), dtype=bool)
        for y, x, _, _ in bad:
            own[y // F * F:y // F * F + F, x // F * F:x // F * F + F] = True
        for kind in ("edge", "albedo", "both"):
            A2, E2 = A.copy(), E.copy()
            for y, x, c, value in bad:
                if kind in ("albedo", "both"):
                    A2[y, x, c] = value
                if kind in ("edge", "both"):
                    E2[y, x, c] = value
            g = uh.guides_for(kind, (A2, n_a), (E2, n_e))
            got = rt.upsample_host(low, spp, (w, h), factor=F, **g)
            assert uh.same_bits(got, uh.upsample(low, spp, (w, h), factor=F, **g))
            assert np.isfinite(got[~own]).all(), (F, kind)


def test_no_guide_and_one_dyadic_value_gives_that_value(rt):
    for F in (2, 4):
        for w, h in ((13, 7), (2, 2), (65, 17)):
            lh, lw = uh.low_size(h, F), uh.low_size(w, F)
            low = np.full((lh, lw, 3), 0.8125) * np.array([1.0, 4.0, -0.5])
            got = rt.upsample_host(low, 1, (w, h), factor=F)
            assert uh.same_bits(got, np.broadcast_to(low[0, 0], (h, w, 3))), (F, w, h)
            assert uh.same_bits(rt.upsample_host(low * 8.0, 8, (w, h), factor=F), got), "sums with a dyadic count"


def test_a_constant_guide_changes_nothing(rt):
    w, h = 13, 7
    for F in uh.FACTORS:
        low, spp, alb, edge = uh.inputs(w, h, F, seed=41, special=True)
        plain = rt.upsample_host(low, spp, (w, h), factor=F)
        flat = np.full((h, w, 3), 1.0) * np.array([0.5, 1.0, 0.0]) * 4.0
        assert uh.same_bits(rt.upsample_host(low, spp, (w, h), factor=F, edge_sum=flat, edge_spp=4), plain), F
        # an albedo guide of A = n_a everywhere: d = 1, R = C, ea = 1 and r * 1 = r
        ones = np.full((h, w, 3), 3.0)
        assert uh.same_bits(rt.upsample_host(low, spp, (w, h), factor=F, albedo_sum=ones, albedo_spp=3), plain), F
        assert uh.same_bits(rt.upsample_host(low, spp, (w, h), factor=F, albedo_sum=ones, albedo_spp=3, edge_sum=flat, edge_spp=4), plain), F


def _own_side(w, F, x0):
    """per column: True where every in-frame tap's low block lies wholly on the column's own side of x0"""
    lw = uh.low_size(w, F)
    i0, _ = uh.footprint(w, F)
    out = np.zeros(w, dtype=bool)
    for x in range(w):
        taps = [I for I in range(i0[x] - 1, i0[x] + 3) if 0 <= I < lw]
        out[x] = all((F * I + F <= x0) if x < x0 else (F * I >= x0) for I in taps)
    return out


def test_taps_of_the_pixels_own_surface_give_the_plain_tent(rt):
    """two surfaces, the low frame any values: a pixel whose in-frame taps all carry its own ID colour takes the plain tent's bits"""
    w, h, x0 = 24, 9, 12
    for F in uh.FACTORS:
        low, spp, _, _ = uh.inputs(w, h, F, seed=43)
        _, _, edge = uh.step_case(w, h, F, x0)
        plain = rt.upsample_host(low, spp, (w, h), factor=F)
        guided = rt.upsample_host(low, spp, (w, h), factor=F, edge_sum=edge, edge_spp=1)
        own = _own_side(w, F, x0)
        assert own.any() and not own.all()
        assert uh.same_bits(guided[:, own], plain[:, own]) and not uh.same_bits(guided[:, ~own], plain[:, ~own]), F


@pytest.mark.parametrize("F,x0", [(2, 5), (2, 9), (4, 5), (4, 9)])
def test_the_edge_guide_keeps_a_step_sharper_than_the_plain_tent(rt, F, x0):
    w, h = 24, 8
    truth, low, edge = uh.step_case(w, h, F, x0)
    tent = rt.upsample_host(low, 1, (w, h), factor=F)
    guided = rt.upsample_host(low, 1, (w, h), factor=F, edge_sum=edge, edge_spp=1)
    assert uh.same_bits(tent, uh.upsample(low, 1, (w, h), factor=F)) and uh.same_bits(guided, uh.upsample(low, 1, (w, h), edge_sum=edge, edge_spp=1, factor=F))
    own = _own_side(w, F, x0)
    assert own.any()
    assert np.array_equal(guided[:, own], truth[:, own]), "taps of the pixel's own side only: exactly 1 or 0"
    err_tent, err_guided = np.abs(tent - truth), np.abs(guided - truth)
    assert (err_guided[:, ~own] <= err_tent[:, ~own]).all() and (err_guided[:, ~own] < err_tent[:, ~own]).any()


def test_wrong_frames_are_refused(rt):
    with pytest.raises(rt.RtError):
        rt.upsample_host(np.zeros((4, 4)), 1, (8, 8))
    with pytest.raises(rt.RtError):
        rt.upsample_host(np.zeros((4, 4, 3)), 1, (9, 8))                       # 9 x 8 at factor 2 needs a 5 x 4 low frame
    with pytest.raises(rt.RtError):
        rt.upsample_host(np.zeros((4, 4, 3)), 1, (8, 8), edge_sum=np.zeros((4, 4, 3)), edge_spp=1)
    with pytest.raises(rt.RtError, match="factor"):
        rt.upsample_host(np.zeros((2, 2, 3)), 1, (8, 8), factor=5)
    with pytest.raises(rt.RtError, match="edge_spp"):
        rt.upsample_host(np.zeros((4, 4, 3)), 1, (8, 8), edge_sum=np.zeros((8, 8, 3)), edge_spp=0)
