"""The host mirror of the tone-mapping stage (rth_tonemap, rth_log_average_luminance; no GPU) against the numpy restatement of
include/rt_amd.h "tone mapping" in tests/tonemap_helpers.py: bytes for the three operators over the edge values, the clamp identity
against rth_resolve_rgb8, and the log-average's tree at every size where its shape changes."""
import math

import numpy as np
import pytest

import tonemap_helpers as th

NAMES = {th.CLAMP: "clamp", th.REINHARD: "reinhard", th.ACES: "aces"}


@pytest.fixture(scope="module")
def frames():
    """one frame per size of the byte tests, shared and never written"""
    out = {(w, h): th.value_frame(w, h, shift=w) for w, h in th.SIZES[:5]}
    for f in out.values():
        f.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def radiance():
    """the log-average inputs with their restated (log_mean, count), computed once"""
    out = {}
    for w, h in th.SIZES:
        f = th.radiance_frame(w, h, seed=w + h)
        f.setflags(write=False)
        out[(w, h)] = (f, th.log_average(f, 1))
    return out


@pytest.mark.parametrize("op", th.OPS, ids=lambda o: NAMES[o])
@pytest.mark.parametrize("white", [th.INF, 4.0])
def test_the_mirror_gives_the_restated_bytes(rt, frames, op, white):
    for (w, h), f in frames.items():
        for exposure in (1.0, 1.7):
            want = th.expected_rgb8(f, 1, op=op, scale=exposure, white=white)
            rgb, rgba = rt.tonemap_host(f, 1, rgba8=True, op=op, exposure=exposure, white=white)
            assert np.array_equal(rgb, want), (w, h, exposure)
            assert np.array_equal(rgba, th.rgba_of(want)), (w, h, exposure)


@pytest.mark.parametrize("op", th.OPS, ids=lambda o: NAMES[o])
def test_sums_with_a_count_and_with_a_map_divide_as_the_resolve_stages_do(rt, frames, op):
    f = frames[(16, 16)]
    want = th.expected_rgb8(f, 3, op=op, scale=0.5)
    assert np.array_equal(rt.tonemap_host(f, 3, op=op, exposure=0.5), want)
    spp_map = th.spp_map_for(16, 16)
    want = th.expected_rgb8(f, 1, spp_map, op=op, scale=0.5)
    assert np.array_equal(rt.tonemap_host(f, 1, spp_map=spp_map, op=op, exposure=0.5), want)


def test_the_operators_do_what_they_are_for(rt):
    """the restatement itself, against numbers worked out by hand: Reinhard maps `white` to 1, ACES' fit at 1 is 2.54 / 3.16, and what
    is not in (0, inf) is not touched"""
    assert th.operator(th.REINHARD, np.array([4.0]), white=4.0)[0] == (4.0 * (1.0 + 4.0 / 16.0)) / 5.0 == 1.0
    assert th.operator(th.REINHARD, np.array([1.0]))[0] == 0.5
    assert th.operator(th.ACES, np.array([1.0]))[0] == (2.51 + 0.03) / ((2.43 + 0.59) + 0.14)
    for op in th.OPS:
        y = th.operator(op, np.array([0.0, -0.0, -3.0, th.INF, -th.INF, float("nan")]), white=4.0)
        assert y[0] == 0.0 and not np.signbit(y[0]) and np.signbit(y[1]) and y[2] == -3.0 and y[3] == th.INF and y[4] == -th.INF and np.isnan(y[5])
    # 15, a stock emitter's radiance, is clipped flat by the clamp and kept apart from 4 by the two curves
    f = np.array([[[15.0, 4.0, 1.0]]])
    assert rt.tonemap_host(f, 1, op="clamp")[0, 0].tolist() == [255, 255, 255]
    for op in ("reinhard", "aces"):
        r, g, b = rt.tonemap_host(f, 1, op=op, exposure=0.25)[0, 0].tolist()
        assert r > g > b, (op, r, g, b)


def test_clamp_at_exposure_one_is_the_existing_output_stage(rt, frames):
    for (w, h), f in frames.items():
        for spp in (1, 3, 10):
            assert np.array_equal(rt.tonemap_host(f, spp), rt.resolve_rgb8_host(w, h, spp, f)), (w, h, spp)


def test_log_mean_and_count_are_the_trees(rt, radiance):
    for (w, h), (f, (want_mean, want_count)) in radiance.items():
        log_mean, lavg, count, zero = rt.log_average_luminance_host(f, 1)
        assert count == want_count and 0 < want_count <= w * h, (w, h)
        assert want_count < w * h or w * h < 8, "some pixels must not count"
        assert log_mean.hex() == float(want_mean).hex(), (w, h)
        assert th.ulps(lavg, math.exp(log_mean)) <= 4.0, (w, h, lavg)  # one ulp each for rt_exp and libm's exp, doubled
        assert zero == 0.0


def test_sums_forms_feed_the_tree_their_means(rt):
    w, h = 257, 3
    f = th.radiance_frame(w, h, seed=9) * 3.0
    want_mean, want_count = th.log_average(f, 3, delta=1e-2)
    got = rt.log_average_luminance_host(f, 3, delta=1e-2)
    assert (got[0].hex(), got[2]) == (float(want_mean).hex(), want_count)
    spp_map = th.spp_map_for(w, h)
    want_mean, want_count = th.log_average(f, 1, spp_map)
    got = rt.log_average_luminance_host(f, 1, spp_map=spp_map)
    assert (got[0].hex(), got[2]) == (float(want_mean).hex(), want_count)


def test_the_input_tells_summation_orders_apart(radiance):
    """a test of the tree must use terms whose in-order sum is another double than the tree's"""
    f, _ = radiance[(65537, 1)]
    terms, counts = th.log_terms(th.means(f, 1), 1e-4)
    in_order = 0.0
    for t in terms.tolist():
        in_order = in_order + t
    T, count = th.tree(terms, counts)
    assert count == int(counts.sum())
    assert in_order != T
    assert abs(in_order - T) < 1e-6 * abs(T)  # (the same sum, another rounding)


def test_auto_exposure_is_the_scale_from_the_log_average(rt, radiance):
    f, _ = radiance[(257, 255)]
    log_mean, lavg, count, _ = rt.log_average_luminance_host(f, 1)
    for op in th.OPS:
        scale = th.scale_of(1.5, 0.18, lavg, count)
        want = th.expected_rgb8(f, 1, op=op, scale=scale)
        assert np.array_equal(rt.tonemap_host(f, 1, op=op, exposure=1.5, auto_key=0.18), want), op
    # the point of it: the log-average of the exposed frame lands on the key
    assert math.isclose(lavg * th.scale_of(1.0, 0.18, lavg, count), 0.18, rel_tol=1e-12)


def test_a_frame_where_nothing_counts_keeps_the_exposure(rt):
    f = np.full((3, 5, 3), float("nan"))
    f[1, 2] = (-1.0, 0.0, 0.0)    # finite, but its luminance is negative
    f[0, 0] = (th.INF, 1.0, 1.0)
    assert rt.log_average_luminance_host(f, 1) == (0.0, 0.0, 0.0, 0.0)
    g = th.value_frame(5, 3)
    g[..., 1] = float("nan")      # every pixel has a NaN: none counts, the other channels still get their bytes
    assert rt.log_average_luminance_host(g, 1)[2] == 0.0
    assert np.array_equal(rt.tonemap_host(g, 1, op="aces", exposure=1.7, auto_key=0.18), rt.tonemap_host(g, 1, op="aces", exposure=1.7))


def test_the_mirror_refuses_what_the_device_call_refuses(rt):
    f = np.ones((2, 2, 3))
    nan = float("nan")
    for kw, field in ((dict(op=3), "op"), (dict(op=-1), "op"), (dict(exposure=0.0), "exposure"), (dict(exposure=th.INF), "exposure"),
                      (dict(exposure=nan), "exposure"), (dict(delta=0.0), "delta"), (dict(delta=nan), "delta"), (dict(auto_key=-0.1), "auto_key"),
                      (dict(auto_key=th.INF), "auto_key"), (dict(white=0.0), "white"), (dict(white=nan), "white"), (dict(struct_size=12), "struct_size")):
        with pytest.raises(rt.RtError, match=field):
            rt.tonemap_host(f, 1, **kw)
    with pytest.raises(rt.RtError, match="spp"):
        rt.tonemap_host(f, 0)
    with pytest.raises(rt.RtError, match="delta"):
        rt.log_average_luminance_host(f, 1, delta=-1.0)
    assert rt.tonemap_host(f, 1, op="reinhard", white=th.INF).shape == (2, 2, 3)
