"""rt_denoise_guided_mean_device, rt_denoise_guided_mean_spatial_device and rt_denoise_guided_views_device (rt_denoise.hip:
denoise_prepare_kernel<DN_EDGES | DN_BOTH, Means>, denoise_prepare_spatial_kernel<R, DN_EDGES | DN_BOTH>, then the à-trous kernels as
they are): the device held to the numpy restatement of tests/guided_routes_helpers.py bit for bit (u64 view), the RGBA8 bytes to
display().

Frames: 37 x 19 (2 x 3 tiles of 32 x 8, ragged on both sides), 32 x 8 (exactly one tile), 5 x 3 and 1 x 1 (narrower than every
halo); K = 1..6 at 37 x 19 (strides 1 and 2: the LDS kernel; 4 .. 32: the global kernel, its taps leaving the frame); R = 1, 2, 3.
Inputs are live_denoise_helpers.synthetic_means / synthetic_albedo_mean and guided_helpers.synthetic_edges as means, whose guide has
anti-aliased borders (0 < tg < 1), a black strip and NaN and +-inf entries: such a pixel comes out unchanged and is never a tap or a
window member.  With a constant guide each form equals the existing unguided entry point on the device."""
import numpy as np
import pytest

import albedo_helpers
import denoise_helpers
import guided_helpers as gh
import guided_routes_helpers as grh
import live_denoise_helpers as ldh
from adaptive_helpers import assert_bits

pytestmark = pytest.mark.gpu

SIZES = [(37, 19), (32, 8), (5, 3), (1, 1)]
_frames = {}


def frames(w, h):
    """(M, M2, A, E): shared, read-only; M2 after 8 samples (any count may be claimed for it: the definition reads it as n says)"""
    if (w, h) not in _frames:
        M, M2, _ = ldh.synthetic_means(w, h, 1000 * w + h)
        A = np.array(ldh.synthetic_albedo_mean(w, h, 77 * w + h))
        E = np.array(grh.synthetic_edge_mean(w, h, 31 * w + h))
        M, M2 = np.array(M), np.array(M2)
        if w > 32:  # not-valid guide pixels where the tiling can go wrong: a tile's corner and the column a halo stages
            E[7, 31, 0] = np.nan
            E[8, 32, 2] = -np.inf
            E[0, 0, 1] = np.inf
        for a in (M, M2, A, E):
            a.setflags(write=False)
        _frames[(w, h)] = (M, M2, A, E)
    return _frames[(w, h)]


def check(rt, got, want, what):
    out, rgba = got
    assert_bits(out, want, what)
    assert np.array_equal(rgba, grh.display(rt, want)), what + ": the display bytes"


@pytest.mark.parametrize("albedo", [False, True])
@pytest.mark.parametrize("w, h, k", [(37, 19, k) for k in range(1, 7)] + [(w, h, 4) for w, h in SIZES[1:]])
def test_the_means_form_equals_the_restatement(rt, w, h, k, albedo):
    M, M2, A, E = frames(w, h)
    A = A if albedo else None
    want = grh.denoise_guided_mean(M, M2, 8, E, A, iterations=k)
    check(rt, rt.denoise_guided_mean(M, M2, 8, E, albedo_mean=A, rgba8=True, iterations=k), want, f"{w}x{h} K={k}")
    bad = ~np.isfinite(E).all(axis=2)
    if w * h >= 15:
        assert bad.any()
    assert_bits(want[bad], M[bad], "a pixel with a non-finite guide comes out unchanged")


@pytest.mark.parametrize("albedo", [False, True])
@pytest.mark.parametrize("samples", [1, 2, 7])
def test_the_means_form_at_other_sample_counts(rt, samples, albedo):
    M, M2, A, E = frames(37, 19)
    A = A if albedo else None
    want = grh.denoise_guided_mean(M, M2, samples, E, A, sigma_edge=0.75)
    check(rt, rt.denoise_guided_mean(M, M2, samples, E, albedo_mean=A, rgba8=True, sigma_edge=0.75), want, f"samples={samples}")
    if samples == 1:
        assert_bits(want, M, "one sample: d_mean, bit for bit")


@pytest.mark.parametrize("albedo", [False, True])
@pytest.mark.parametrize("w, h, R", [(37, 19, R) for R in (1, 2, 3)] + [(w, h, R) for w, h in SIZES[1:] for R in (1, 3)])
def test_the_spatial_form_equals_the_restatement_without_m2(rt, w, h, R, albedo):
    M, _, A, E = frames(w, h)
    A = A if albedo else None
    want = grh.denoise_guided_mean_spatial(M, None, 1, E, A, window_radius=R)
    check(rt, rt.denoise_guided_mean_spatial(M, None, 1, E, albedo_mean=A, rgba8=True, window_radius=R), want, f"{w}x{h} R={R}")
    bad = ~np.isfinite(E).all(axis=2)
    assert_bits(want[bad], M[bad], "a pixel with a non-finite guide comes out unchanged")


@pytest.mark.parametrize("albedo", [False, True])
def test_the_spatial_form_below_a_higher_threshold_and_with_other_parameters(rt, albedo):
    M, M2, A, E = frames(37, 19)
    A = A if albedo else None
    kw = dict(spatial_below=4, window_radius=2, iterations=3, sigma_edge=0.3)
    want = grh.denoise_guided_mean_spatial(M, None, 3, E, A, **kw)
    check(rt, rt.denoise_guided_mean_spatial(M, None, 3, E, albedo_mean=A, rgba8=True, **kw), want, "3 samples below 4")


@pytest.mark.parametrize("albedo", [False, True])
def test_the_spatial_form_at_its_threshold_is_the_means_form(rt, albedo):
    M, M2, A, E = frames(37, 19)
    A = A if albedo else None
    for samples, below in ((2, 2), (8, 2), (1, 1)):
        got = rt.denoise_guided_mean_spatial(M, M2, samples, E, albedo_mean=A, rgba8=True, spatial_below=below, window_radius=3)
        ref = rt.denoise_guided_mean(M, M2, samples, E, albedo_mean=A, rgba8=True)
        assert_bits(got[0], ref[0], f"samples={samples}, spatial_below={below}")
        assert np.array_equal(got[1], ref[1])
        check(rt, got, grh.denoise_guided_mean(M, M2, samples, E, A), "the restatement")
    assert_bits(rt.denoise_guided_mean_spatial(M, M2, 1, E, albedo_mean=A, spatial_below=1), M, "one sample, no spatial route: d_mean")


@pytest.mark.parametrize("R", [1, 2, 3])
def test_the_two_surface_step_on_the_device(rt, R):
    M, E = grh.step_frames(37, 19)
    out, rgba = rt.denoise_guided_mean_spatial(M, None, 1, E, rgba8=True, window_radius=R)
    assert_bits(out, M, "the edge-aware window sees no spread: the output is the input")
    assert np.array_equal(rgba, grh.display(rt, M))
    plain = rt.denoise_mean_spatial(M, None, 1, window_radius=R)
    assert (plain != M).any(), "the unguided window spans the border and blurs it"


def views_inputs(n_views=3, w=33, h=9):
    stack = [denoise_helpers.synthetic(w, h, 10 + v) for v in range(n_views)]
    S, Q = np.stack([s[0] for s in stack]), np.stack([s[1] for s in stack])
    A = np.stack([albedo_helpers.synthetic_albedo(w, h, 20 + v, n_a=4)[0] for v in range(n_views)])
    E = np.stack([gh.synthetic_edges(w, h, 30 + v)[0] for v in range(n_views)])
    return S, Q, stack[0][2], A, 4, E, 4


@pytest.mark.parametrize("albedo", [False, True])
def test_each_view_of_a_stack_equals_the_single_frame_call(rt, albedo):
    S, Q, n, A, n_a, E, n_e = views_inputs()
    A = A if albedo else None
    assert not np.array_equal(S[0], S[1]) and not np.array_equal(E[1], E[2])
    got = rt.denoise_guided_views(S, Q, n, E, n_e, albedo_sum=A, albedo_spp=n_a, rgba8=True, iterations=5)
    check(rt, (got[0].reshape(-1, 33, 3), got[1].reshape(-1, 33, 4)),
          grh.denoise_guided_views(S, Q, n, E, n_e, A, n_a, iterations=5).reshape(-1, 33, 3), "the stack")
    for v in range(len(S)):
        one = rt.denoise_guided(S[v], Q[v], n, E[v], n_e, albedo_sum=None if A is None else A[v], albedo_spp=n_a, rgba8=True, iterations=5)
        assert_bits(got[0][v], one[0], f"view {v}")
        assert np.array_equal(got[1][v], one[1]), f"view {v}: the display bytes"


@pytest.mark.parametrize("albedo", [False, True])
def test_no_tap_crosses_into_a_neighbouring_view(rt, albedo):
    S, Q, n, A, n_a, E, n_e = views_inputs()
    A = A if albedo else None
    want = rt.denoise_guided_views(S, Q, n, E, n_e, albedo_sum=A, albedo_spp=n_a, iterations=6)[1]

    def walled(x):
        y = np.full_like(x, 1e300)
        y[1] = x[1]
        return y
    got = rt.denoise_guided_views(walled(S), walled(Q), n, walled(E), n_e, albedo_sum=None if A is None else walled(A), albedo_spp=n_a, iterations=6)[1]
    assert_bits(got, want, "the middle view between two views of 1e300")


def test_a_constant_guide_leaves_every_route_as_it_was(rt):
    M, M2, A, _ = frames(37, 19)
    G = grh.constant_guide(37, 19)
    assert_bits(rt.denoise_guided_mean(M, M2, 8, G), rt.denoise_mean(M, M2, 8), "means")
    assert_bits(rt.denoise_guided_mean(M, M2, 8, G, albedo_mean=A), rt.denoise_albedo_mean(M, M2, 8, A), "means, albedo")
    for R in (1, 3):
        assert_bits(rt.denoise_guided_mean_spatial(M, None, 1, G, window_radius=R), rt.denoise_mean_spatial(M, None, 1, window_radius=R), f"spatial R={R}")
        assert_bits(rt.denoise_guided_mean_spatial(M, None, 1, G, albedo_mean=A, window_radius=R),
                    rt.denoise_albedo_mean_spatial(M, None, 1, A, window_radius=R), f"spatial R={R}, albedo")
    S, Q, n, A, n_a, E, n_e = views_inputs()
    G = np.stack([grh.constant_guide(33, 9) * n_e] * len(S))
    assert_bits(rt.denoise_guided_views(S, Q, n, G, n_e), rt.denoise_views(S, Q, n), "views")
    assert_bits(rt.denoise_guided_views(S, Q, n, G, n_e, albedo_sum=A, albedo_spp=n_a), rt.denoise_albedo_views(S, Q, n, A, n_a), "views, albedo")
