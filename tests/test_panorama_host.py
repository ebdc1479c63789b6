"""Panoramas on the CPU: the cube-face cameras and the host mirror rth_panorama against numpy restatements of the header, bit for bit; the
tables against numpy's sine and cosine; face choice at exact ties; cameras and resampler agreeing on which way every face looks; and the
header's consequences."""
import numpy as np
import pytest

import panorama_helpers as ph


@pytest.mark.parametrize("F,g", ph.FACES)
def test_the_six_cameras_are_the_headers_arithmetic_bit_for_bit(rt, F, g):
    like = rt.Camera(image_width=7, image_height=5, samples_per_pixel=9, max_depth=11, defocus_angle=0.6)
    like.background.x, like.background.y, like.background.z = 0.25, 0.5, 0.75
    like.center.x, like.center.y, like.center.z = 1.0, 2.0, 3.0
    like.defocus_disk_u.x = like.defocus_disk_v.y = 0.125
    cams = rt.cube_face_cameras(like, ph.CENTER, face_size=F, guard=g)
    want = ph.cameras_ref(ph.CENTER, F, g)
    for f in range(6):
        c = cams[f]
        assert (c.image_width, c.image_height, c.samples_per_pixel, c.max_depth) == (F, F, 9, 11)
        assert np.array_equal(ph.vec(c.background), [0.25, 0.5, 0.75])
        assert c.defocus_angle == 0.0 and not ph.vec(c.defocus_disk_u).any() and not ph.vec(c.defocus_disk_v).any()
        for field in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v"):
            assert np.array_equal(ph.bits(ph.vec(getattr(c, field))), ph.bits(want[f][field])), (f, field)
    delta = 2.0 / (F - 2 * g)
    for a, b in ((0, 1), (2, 3), (4, 5)):
        fwd = [np.cross(ph.vec(cams[k].pixel_delta_u), -ph.vec(cams[k].pixel_delta_v)) / (delta * delta) for k in (a, b)]   # r x u = -n
        assert np.array_equal(fwd[0], -fwd[1]) and np.abs(fwd[0]).sum() == 1.0
    # a null centre is like's
    own = rt.cube_face_cameras(like, None, face_size=F, guard=g)
    assert all(np.array_equal(ph.vec(own[f].center), [1.0, 2.0, 3.0]) for f in range(6))


@pytest.mark.parametrize("W,H", ph.SIZES + ((64, 32), (6, 4)))
def test_the_tables_are_numpys_and_the_hemispheres_mirror_each_other(rt, W, H):
    t = rt.panorama_tables(W, H)
    assert t.shape == (2 * W + 2 * H,)
    lam = ((np.arange(W, dtype=np.float64) + 0.5) / W - 0.5) * (2.0 * np.pi)
    phi = (0.5 - (np.arange(H, dtype=np.float64) + 0.5) / H) * np.pi
    for got, want in ((t[0:2 * W:2], np.sin(lam)), (t[1:2 * W:2], np.cos(lam)), (t[2 * W::2], np.sin(phi)), (t[2 * W + 1::2], np.cos(phi))):
        print(W, H, float(np.max(np.abs(got - want))))
        assert np.max(np.abs(got - want)) <= 1e-15
    s, c = t[2 * W::2], t[2 * W + 1::2]
    assert np.array_equal(s, -s[::-1]) and np.array_equal(ph.bits(c), ph.bits(c[::-1]))
    assert np.array_equal(ph.bits(s[: H // 2]), ph.bits(-s[::-1][: H // 2]))
    if H % 2:
        assert s[H // 2] == 0.0 and c[H // 2] == 1.0


@pytest.mark.parametrize("spp", (3, 1))
@pytest.mark.parametrize("F,g", ph.FACES)
@pytest.mark.parametrize("W,H", ph.SIZES)
def test_the_mirror_is_the_numpy_restatement_bit_for_bit(rt, W, H, F, g, spp):
    faces = ph.random_faces(F, 100 * F + g, spp)
    t = rt.panorama_tables(W, H)
    got = rt.panorama_host(W, H, faces, g, spp, tables=t)
    assert np.array_equal(ph.bits(got), ph.bits(ph.resample_ref(W, H, t, faces, g, spp)))
    assert np.isfinite(got).all()


@pytest.mark.parametrize("F,g", ph.FACES)
def test_exact_ties_choose_the_face_the_header_prescribes(rt, F, g):
    t, W, H, want = ph.tie_tables()
    got = rt.panorama_host(W, H, ph.index_faces(F), g, 1, tables=t)
    assert np.array_equal(got, np.repeat(want[..., None].astype(np.float64), 3, axis=2))
    assert np.array_equal(ph.face_map(t, W, H)[0], want)


@pytest.mark.parametrize("F,g", ((10, 1), (12, 2)))
def test_cameras_and_resampler_agree_on_every_faces_orientation(rt, F, g):
    """A face whose texels hold their own direction (over its forward component's magnitude) is linear in the face coordinates, guard ring
    included, so the bilinear filter reproduces it: every output pixel must come back as d / m of its own direction."""
    W, H = 64, 32
    like = rt.Camera()
    cams = rt.cube_face_cameras(like, (0.0, 0.0, 0.0), face_size=F, guard=g)
    faces = np.zeros((6, F, F, 3))
    i = np.arange(F, dtype=np.float64)
    for f in range(6):
        p00, du, dv = (ph.vec(getattr(cams[f], n)) for n in ("pixel00_loc", "pixel_delta_u", "pixel_delta_v"))
        d = p00[None, None, :] + i[None, :, None] * du[None, None, :] + i[:, None, None] * dv[None, None, :] - ph.vec(cams[f].center)
        faces[f] = d / np.abs(d[..., ph.AXES[f][0][0]])[..., None]
    assert np.array_equal(faces, ph.direction_faces(F, g))
    t = rt.panorama_tables(W, H)
    got = rt.panorama_host(W, H, faces, g, 1, tables=t)
    err = float(np.max(np.abs(got - ph.own_direction(t, W, H))))
    print(F, g, err)
    assert err <= 1e-12


@pytest.mark.parametrize("F,g", ph.FACES)
def test_a_constant_stack_comes_back_to_the_bit(rt, F, g):
    for value, spp in ((0.1, 1), (3.3, 1), (-7.25e-3, 1), (0.3, 3)):
        faces = np.full((6, F, F, 3), value)
        got = rt.panorama_host(65, 33, faces, g, spp)
        assert np.array_equal(ph.bits(got), ph.bits(np.full((33, 65, 3), np.float64(value) * (np.float64(1.0) / np.float64(spp)))))


def test_with_two_guard_texels_the_outermost_ring_is_never_read(rt):
    F, g, W, H = 9, 2, 130, 65
    faces = np.array(ph.random_faces(F, 5, 1))
    clean = rt.panorama_host(W, H, faces, g, 1)
    faces[:, 0, :, :] = faces[:, -1, :, :] = faces[:, :, 0, :] = faces[:, :, -1, :] = np.nan
    assert np.array_equal(ph.bits(rt.panorama_host(W, H, faces, g, 1)), ph.bits(clean))
    assert not ph.tapped(rt.panorama_tables(W, H), W, H, F, g)[:, :, :, [0, -1], :].any()


@pytest.mark.parametrize("value", (np.nan, np.inf))
def test_a_non_finite_texel_shows_in_exactly_the_pixels_that_tap_it(rt, value):
    F, g, W, H = 6, 1, 96, 48
    t = rt.panorama_tables(W, H)
    hit = ph.tapped(t, W, H, F, g)
    clean = rt.panorama_host(W, H, ph.random_faces(F, 9, 1), g, 1, tables=t)
    for f, y, x in ((0, 2, 3), (3, 1, 1), (5, 4, 0), (2, 0, 5)):
        faces = np.array(ph.random_faces(F, 9, 1))
        faces[f, y, x, 1] = value
        got = rt.panorama_host(W, H, faces, g, 1, tables=t)
        bad = ~np.isfinite(got[:, :, 1])
        assert np.array_equal(bad, hit[:, :, f, y, x]), (f, y, x)
        assert f != 0 or bad.any()
        assert np.array_equal(ph.bits(got[:, :, [0, 2]]), ph.bits(clean[:, :, [0, 2]]))
        assert np.array_equal(ph.bits(got[~bad]), ph.bits(clean[~bad]))


def test_a_tap_of_weight_zero_still_carries_a_non_finite_texel(rt):
    """dx = 1, dy = 0, dz = -0 looks at the centre of face 0; with F = 5 that is texel (2, 2) exactly, fx = fy = 0, and the three other
    taps have weight 0: 0 * NaN is NaN, so they show all the same."""
    t, W, H, _ = ph.tie_tables()
    F, g = 5, 1
    _, x0, y0, fx, fy = ph.taps(t, W, H, F, g)
    assert (x0[1, 10], y0[1, 10], fx[1, 10], fy[1, 10]) == (2, 2, 0.0, 0.0)
    for y, x in ((2, 3), (3, 2), (3, 3)):
        faces = np.array(ph.random_faces(F, 3, 1))
        faces[0, y, x, :] = np.nan
        got = rt.panorama_host(W, H, faces, g, 1, tables=t)
        assert np.isnan(got[1, 10]).all(), (y, x)
