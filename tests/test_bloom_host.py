"""The host mirror of bloom (rth_bloom; no GPU) against the numpy restatement of include/rt_amd.h "bloom" in tests/bloom_helpers.py, bit
for bit: every listed frame in the three input forms, the impulse against a hand-written table, the identity without a bright pixel,
non-finite pixels, and inputs on which a wrong accumulation order or a wrong pass structure gives other bits."""
import numpy as np
import pytest

import bloom_helpers as bh


@pytest.fixture(scope="module")
def frames():
    """one frame per shape, shared and never written"""
    out = {(w, h): bh.frame(w, h, seed=w + h) for w, h, _ in bh.SHAPES + bh.LONG}
    for f in out.values():
        f.setflags(write=False)
    return out


@pytest.mark.parametrize("w,h,levels", bh.SHAPES + bh.LONG, ids=lambda v: str(v))
def test_the_mirror_gives_the_restated_bits(rt, frames, w, h, levels):
    f = frames[(w, h)]
    assert not np.isfinite(f).all() and (f < 0).any()
    kw = dict(levels=levels, threshold=0.5, strength=0.7)
    spp_map = bh.spp_map_for(w, h)
    for name, spp, smap in (("sums", 7, None), ("map", 1, spp_map), ("means", 1, None)):
        want = bh.bloom(f, spp, smap, **kw)
        got = rt.bloom_host(f, spp, spp_map=smap, **kw)
        assert bh.same_bits(got, want), (name, int((got.view(np.uint64) != want.view(np.uint64)).sum()))
    if w * h > 1:
        assert not bh.same_bits(bh.bloom(f, 1, **kw), bh.means(f, 1)), "the frame must glow"
    assert bh.same_bits(rt.bloom_host(f, 1), bh.bloom(f, 1, **bh.DEFAULTS))   # the defaults are the header's


def test_an_impulse_gives_the_outer_products_of_the_dyadic_taps(rt):
    f = np.zeros((33, 33, 3))
    f[16, 16] = (1.0, 1.0, 1.0)
    got = rt.bloom_host(f, 1, levels=2, threshold=0.0, strength=1.0)
    h1 = np.array([1, 4, 6, 4, 1]) / 16.0                                        # level 1: h
    h2 = np.array([1, 4, 10, 20, 31, 40, 44, 40, 31, 20, 10, 4, 1]) / 256.0      # level 2: h at stride 2 over h, worked out by hand
    glow = np.zeros((33, 33))
    glow[14:19, 14:19] += np.outer(h1, h1)
    glow[10:23, 10:23] += np.outer(h2, h2)
    want = f + (glow / 2.0)[..., None]
    assert np.array_equal(got, want)
    assert got[16, 16, 0] == 1.0 + (36.0 / 256.0 + 44.0 * 44.0 / 65536.0) / 2.0 and got[0, 0, 0] == 0.0 and got[16, 22, 1] == (44.0 / 65536.0) / 2.0
    assert np.array_equal(bh.bloom(f, 1, levels=2, threshold=0.0, strength=1.0), want)


def test_without_a_bright_pixel_the_output_is_the_means_bits(rt):
    f = bh.frame(17, 9, seed=3, special=False)
    assert not np.signbit(f[f == 0.0]).any()
    top = float(np.abs(f).max()) * 4.0
    for spp, smap in ((7, None), (1, bh.spp_map_for(17, 9)), (1, None)):
        assert bh.same_bits(rt.bloom_host(f, spp, spp_map=smap, threshold=top, strength=3.0), bh.means(f, spp, smap))
    dark = np.full((5, 4, 3), 0.25)
    assert bh.same_bits(rt.bloom_host(dark, 1), dark)   # the default threshold 1.0: nothing in a dim frame glows


def test_a_non_finite_pixel_does_not_spread_and_keeps_its_class(rt):
    f = np.full((9, 11, 3), 3.0)
    f[4, 5] = (np.nan, 3.0, 3.0)
    f[2, 2] = (3.0, np.inf, 3.0)
    f[6, 8] = (3.0, 3.0, -np.inf)
    got = rt.bloom_host(f, 1, levels=3, threshold=0.5, strength=1.0)
    finite_in = np.isfinite(f)
    assert np.isfinite(got[finite_in]).all()
    assert np.isnan(got[4, 5, 0]) and got[2, 2, 1] == np.inf and got[6, 8, 2] == -np.inf
    assert bh.same_bits(got, bh.bloom(f, 1, levels=3, threshold=0.5, strength=1.0))
    # ... and is no source: its neighbours get what they get when the pixel is black
    g = f.copy()
    g[4, 5] = g[2, 2] = g[6, 8] = 0.0
    black = rt.bloom_host(g, 1, levels=3, threshold=0.5, strength=1.0)
    only_finite = np.isfinite(f).all(axis=2)
    assert bh.same_bits(got[only_finite], black[only_finite])


def test_the_input_tells_accumulation_orders_apart(rt):
    f = bh.frame(17, 9, seed=17, special=False)
    m = bh.means(f, 1)
    B1, B2, B3 = bh.level_frames(bh.bright(m, 0.5), 3)
    left, right = (B1 + B2) + B3, B1 + (B2 + B3)
    assert (left != right).any(), "the input must tell (B1 + B2) + B3 from B1 + (B2 + B3)"
    assert bh.same_bits(bh.accumulate([B1, B2, B3]), left)
    got = rt.bloom_host(f, 1, levels=3, threshold=0.5, strength=0.7)
    assert bh.same_bits(got, m + (0.7 * (left / 3.0)))
    assert not bh.same_bits(got, m + (0.7 * (right / 3.0)))


def test_the_input_tells_the_separable_passes_from_a_25_tap_sum(rt):
    f = bh.frame(17, 9, seed=23, special=False)
    m = bh.means(f, 1)
    B0 = bh.bright(m, 0.5)
    separable, direct = bh.level_frames(B0, 1)[0], bh.blur_2d(B0, 1)
    assert (separable != direct).any() and np.allclose(separable, direct, rtol=1e-9, atol=1e-9 * float(np.abs(direct).max()))
    got = rt.bloom_host(f, 1, levels=1, threshold=0.5, strength=0.7)
    assert bh.same_bits(got, m + (0.7 * (separable / 1.0)))
    assert not bh.same_bits(got, m + (0.7 * (direct / 1.0)))


def test_wrong_frames_are_refused(rt):
    with pytest.raises(rt.RtError):
        rt.bloom_host(np.zeros((4, 4)), 1)
    with pytest.raises(rt.RtError):
        rt.bloom_host(np.zeros((4, 4, 3)), 1, spp_map=np.ones((3, 4), dtype=np.int32))
    with pytest.raises(rt.RtError, match="levels"):
        rt.bloom_host(np.zeros((4, 4, 3)), 1, levels=9)
