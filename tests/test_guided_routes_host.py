"""The numpy restatement of "edge guide on every route" (tests/guided_routes_helpers.py) held to the restatements it grew from, without a
GPU: with a constant guide every form is the unguided form's bit for bit (the header's claim: dg = 0, tg = 1, every valid window pixel
a member), and on the two-surface step — 0.25 beside 0.75, two palette colours split at the same column — the edge-aware spatial V0
is +0.0 at every pixel and the output is the input, where the unguided window has V0 > 0 along the border."""
import numpy as np
import pytest

import albedo_helpers
import denoise_helpers
import guided_routes_helpers as grh
import live_denoise_helpers as ldh
import spatial_denoise_helpers as sdh
from adaptive_helpers import assert_bits

W, H = 37, 19


@pytest.fixture(scope="module")
def inputs():
    M, M2, n = ldh.synthetic_means(W, H, 4242)
    A = np.array(ldh.synthetic_albedo_mean(W, H, 99))
    G = grh.constant_guide(W, H)
    return M, M2, n, A, G


@pytest.mark.parametrize("k", [1, 3, 4])
def test_a_constant_guide_leaves_the_means_form_as_it_was(inputs, k):
    M, M2, n, A, G = inputs
    assert_bits(grh.denoise_guided_mean(M, M2, n, G, iterations=k), ldh.denoise_mean(M, M2, n, iterations=k), "plain")
    assert_bits(grh.denoise_guided_mean(M, M2, n, G, A, iterations=k), ldh.denoise_albedo_mean(M, M2, n, A, iterations=k), "albedo")
    assert_bits(grh.denoise_guided_mean(M, M2, 1, G, A, iterations=k), M, "one sample: the input")


@pytest.mark.parametrize("R", [1, 2, 3])
def test_a_constant_guide_leaves_the_spatial_form_as_it_was(inputs, R):
    M, M2, n, A, G = inputs
    assert_bits(grh.denoise_guided_mean_spatial(M, None, 1, G, window_radius=R), sdh.denoise_mean_spatial(M, None, 1, window_radius=R), "plain")
    assert_bits(grh.denoise_guided_mean_spatial(M, None, 1, G, A, window_radius=R),
                sdh.denoise_albedo_mean_spatial(M, None, 1, A, window_radius=R), "albedo")
    # at the threshold the route is the means form's
    assert_bits(grh.denoise_guided_mean_spatial(M, M2, n, G, A, window_radius=R), ldh.denoise_albedo_mean(M, M2, n, A), "at the threshold")
    C0, V0, valid, g, a, d = grh.prepare_guided_spatial(M, G, A, R=R)
    c0, v0, ok, _, _ = sdh.prepare_albedo_spatial(M, A, grh.DEFAULTS["albedo_floor"], R)
    assert_bits(C0, c0, "C0")
    assert_bits(V0, v0, "V0")
    assert (valid == ok).all()


def test_a_constant_guide_leaves_each_view_as_it_was():
    n_views, w, h = 3, 33, 9
    stack = [denoise_helpers.synthetic(w, h, 10 + v) for v in range(n_views)]
    n = stack[0][2]
    S, Q = np.stack([s[0] for s in stack]), np.stack([s[1] for s in stack])
    A = np.stack([albedo_helpers.synthetic_albedo(w, h, 20 + v, n_a=4)[0] for v in range(n_views)])
    E = np.stack([grh.constant_guide(w, h) * 4.0] * n_views)
    got = grh.denoise_guided_views(S, Q, n, E, 4)
    got_a = grh.denoise_guided_views(S, Q, n, E, 4, A, 4)
    for v in range(n_views):
        assert_bits(got[v], denoise_helpers.denoise(S[v], Q[v], n), f"view {v}")
        assert_bits(got_a[v], albedo_helpers.denoise_albedo(S[v], Q[v], n, A[v], 4), f"view {v}, albedo")


@pytest.mark.parametrize("R", [1, 2, 3])
def test_the_two_surface_step_has_no_spread_inside_a_surface(R):
    M, E = grh.step_frames(W, H)
    C0, V0, valid, g, a, d = grh.prepare_guided_spatial(M, E, R=R)
    assert valid.all()
    assert_bits(V0, np.zeros((H, W)), "the edge-aware V0: +0.0 everywhere")
    assert_bits(grh.denoise_guided_mean_spatial(M, None, 1, E, window_radius=R), M, "the output is the input")
    _, v0, _ = sdh.prepare_spatial(M, R)
    border = np.zeros((H, W), dtype=bool)
    border[:, W // 2 - R: W // 2 + R] = True
    assert (v0[border] > 0.0).all() and (v0[~border] == 0.0).all(), "the unguided window spans the border"


def test_a_non_finite_guide_pixel_is_not_valid_and_no_member():
    M, E = grh.step_frames(W, H)
    M = M + np.linspace(0.0, 1.0, W)[None, :, None]
    E[5, 7, 1] = np.nan
    E[9, 20, 0] = np.inf
    C0, V0, valid, g, a, d = grh.prepare_guided_spatial(M, E, R=1)
    assert not valid[5, 7] and not valid[9, 20] and valid.sum() == W * H - 2
    assert V0[5, 7] == -1.0 and V0[9, 20] == -1.0
    # its neighbours' windows are the frame's with that pixel made invalid in M instead
    M_bad = M.copy()
    M_bad[5, 7, 0] = np.nan
    M_bad[9, 20, 0] = np.nan
    E_ok = grh.step_frames(W, H)[1]
    _, V_ref, _, _, _, _ = grh.prepare_guided_spatial(M_bad, E_ok, R=1)
    assert_bits(V0, V_ref, "V0")
    out = grh.denoise_guided_mean_spatial(M, None, 1, E)
    assert_bits(out[5, 7], M[5, 7], "an invalid pixel comes out unchanged")
