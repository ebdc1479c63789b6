"""Frame metrics without a GPU: the host mirrors rth_frame_error and rth_frame_noise against the numpy restatement of include/rt_amd.h
"frame metrics", bit for bit at every size where the tree changes shape; the special results (psnr = +inf, all zeros, noise = +inf);
the noise call's variance against the denoise helpers' prepare step; and the PFM reader, round trip and refusals."""
import numpy as np
import pytest

import denoise_helpers as dh
import live_denoise_helpers as ldh
import metrics_helpers as mh


@pytest.mark.parametrize("w,h", mh.SIZES)
def test_frame_error_host_is_the_restatement_bit_for_bit(rt, w, h):
    frame, ref = mh.frame_pair(w, h)
    spp_map = mh.spp_map_for(w, h)
    for kw in (dict(spp=1, ref_spp=1), dict(spp=12, ref_spp=48), dict(spp=1, ref_spp=3, spp_map=spp_map), dict(spp=1, ref_spp=1, eps=1e-4, peak=255.0)):
        spp, ref_spp = kw.pop("spp"), kw.pop("ref_spp")
        want = mh.frame_error(frame, spp, ref, ref_spp, **kw)
        got = rt.frame_error_host(frame, spp, ref, ref_spp, **kw)
        assert got["count"] == want["count"]
        assert mh.same_bits(got, want, mh.ERROR_FIELDS), (w, h, kw, got, want)
    if w * h >= 8:
        assert want["count"] == w * h - 3, "the NaN and the two infinities do not count"


@pytest.mark.parametrize("w,h", mh.SIZES)
def test_frame_noise_host_is_the_restatement_bit_for_bit(rt, w, h):
    S, Q = mh.moments(w, h, 8)
    M, M2 = mh.mean_moments(w, h, 8)
    spp_map = mh.spp_map_for(w, h)
    cases = [((S, Q, 8), dict()), ((S, Q, 2), dict(eps=1e-6)), ((S, Q, 8), dict(spp_map=spp_map)), ((M, M2, 8), dict(form="means")),
             ((M, M2, 3), dict(form="means", eps=1.0))]
    for args, kw in cases:
        want = mh.frame_noise(*args, **kw)
        got = rt.frame_noise_host(*args, **kw)
        assert got["count"] == want["count"]
        assert mh.same_bits(got, want, mh.NOISE_FIELDS), (w, h, kw, got, want)
    with_map = mh.frame_noise(S, Q, 8, spp_map=spp_map)
    assert with_map["count"] <= int((spp_map >= 2).sum()), "an entry of 1 in the map does not count"
    if w * h >= 8:
        assert 0 < with_map["count"] < w * h


def test_identical_frames_give_zero_error_and_infinite_psnr(rt):
    frame, _ = mh.frame_pair(17, 9)
    frame = np.where(np.isfinite(frame), frame, 1.0)
    got = rt.frame_error_host(frame, 1, frame, 1)
    assert got["count"] == 17 * 9 and got["psnr"] == mh.INF
    assert all(got[k] == 0.0 for k in ("mse", "rmse", "rel_mse", "mae", "bias", "max_abs"))
    one, ref = mh.frame_pair(1, 1)
    assert rt.frame_error_host(one, 1, ref, 1)["psnr"] == mh.INF, "mse == 0 is reachable in a 1 x 1 frame"


def test_nothing_counting_gives_all_zeros(rt):
    frame = np.full((3, 5, 3), mh.NAN)
    ref = np.ones((3, 5, 3))
    got = rt.frame_error_host(frame, 1, ref, 1)
    assert got == dict.fromkeys(mh.ERROR_FIELDS, 0.0) | {"count": 0}
    assert mh.same_bits(got, mh.frame_error(frame, 1, ref, 1), mh.ERROR_FIELDS)


def test_noise_is_infinite_where_no_pixel_has_two_samples(rt):
    S, Q = mh.moments(17, 9, 1)
    for got in (rt.frame_noise_host(S, Q, 1), rt.frame_noise_host(S, Q, 1, form="means"),
                rt.frame_noise_host(S, Q, 8, spp_map=np.ones((9, 17), dtype=np.int32))):
        assert got == dict(count=0, mean_var=0.0, noise=mh.INF, max_noise=mh.INF)
    assert not (rt.frame_noise_host(S, Q, 1)["noise"] <= 1e300), "a stop test never passes"


def test_the_variance_is_the_denoisers_prepare_variance(rt):
    """The largest channel variance of a pixel is Prepare's V0 ("denoise", "live denoise"), bit for bit: checked on the restatement, which
    the mirror equals above, and through the mirror on one-pixel frames, whose mean_var is that pixel's (var_r + var_g + var_b) / 3."""
    w, h, n = 23, 7, 6
    S, Q = mh.moments(w, h, n)
    for form, (a, b), prep in (("sums", (S, Q), lambda: dh.prepare(S, Q, n)),
                               ("means", mh.mean_moments(w, h, n), None)):
        var, counts = mh.channel_variance(a, b, n, form == "means")
        if form == "sums":
            _, V0, valid = prep()
        else:
            out = ldh.prepare_mean(a, b, n)
            V0, valid = out[1], out[2]
        assert np.array_equal(counts.reshape(h, w), valid)
        biggest = var.max(axis=1).reshape(h, w)
        assert np.array_equal(mh.bits(biggest[valid]), mh.bits(np.asarray(V0)[valid]))
        # one pixel at a time through the mirror
        a3, b3 = np.asarray(a).reshape(-1, 3), np.asarray(b).reshape(-1, 3)
        for p in np.flatnonzero(counts)[:12]:
            got = rt.frame_noise_host(a3[p].reshape(1, 1, 3), b3[p].reshape(1, 1, 3), n, form=form)
            want = ((var[p, 0] + var[p, 1]) + var[p, 2]) / np.float64(3)
            assert mh.bits(got["mean_var"]) == mh.bits(want)


def test_read_pfm_round_trips_in_both_byte_orders(rt, tmp_path):
    frame, _ = mh.frame_pair(13, 5)
    f32 = frame.astype(np.float32)
    want = f32.astype(np.float64)
    path = tmp_path / "little.pfm"
    rt.write_pfm(path, f32)
    got = rt.read_pfm(path)
    assert got.shape == (5, 13, 3) and np.array_equal(mh.bits(got), mh.bits(want))
    big = tmp_path / "big.pfm"
    big.write_bytes(b"PF\n13 5\n1.0\n" + f32[::-1].astype(">f4").tobytes())
    assert np.array_equal(mh.bits(rt.read_pfm(big)), mh.bits(want))
    # white space of any kind between the fields, a scale of another magnitude (not applied), bytes behind the body (not read)
    loose = tmp_path / "loose.pfm"
    loose.write_bytes(b"PF \t13\r\n5 -2.5e0\n" + f32[::-1].astype("<f4").tobytes() + b"tail")
    assert np.array_equal(mh.bits(rt.read_pfm(loose)), mh.bits(want))


@pytest.mark.parametrize("name,header,body_values", [
    ("no magic", b"P6\n2 2\n-1.0\n", 12), ("grey", b"Pf\n2 2\n-1.0\n", 12), ("empty", b"", 0), ("magic only", b"PF", 0),
    ("zero width", b"PF\n0 2\n-1.0\n", 12), ("zero height", b"PF\n2 0\n-1.0\n", 12), ("negative width", b"PF\n-2 2\n-1.0\n", 12),
    ("2^27 pixels", b"PF\n16384 8192\n-1.0\n", 12), ("a product that wraps 32 bits", b"PF\n65536 65536\n-1.0\n", 12),
    ("a product that wraps 64 bits", b"PF\n4294967296 4294967296\n-1.0\n", 12), ("ten digits", b"PF\n0000000002 2\n-1.0\n", 12),
    ("zero scale", b"PF\n2 2\n0.0\n", 12), ("negative zero scale", b"PF\n2 2\n-0.0\n", 12), ("infinite scale", b"PF\n2 2\n-inf\n", 12),
    ("nan scale", b"PF\n2 2\nnan\n", 12), ("no scale", b"PF\n2 2\n", 12), ("garbage behind the scale", b"PF\n2 2\n-1.0x\n", 12),
    ("garbage behind the width", b"PF\n2x 2\n-1.0\n", 12), ("garbage behind the height", b"PF\n2 2;\n-1.0\n", 12),
    ("a fourth field", b"PF\n2 2\n-1.0 7\n", 11), ("a long scale", b"PF\n2 2\n-1." + b"0" * 40 + b"\n", 12),
    ("short body", b"PF\n2 2\n-1.0\n", 11), ("no body", b"PF\n2 2\n-1.0\n", 0), ("header cut in the scale", b"PF\n2 2\n-1.0", 0),
])
def test_read_pfm_refuses_a_malformed_file_with_an_error(rt, tmp_path, name, header, body_values):
    path = tmp_path / "bad.pfm"
    path.write_bytes(header + np.arange(body_values, dtype="<f4").tobytes())
    with pytest.raises(rt.RtError) as e:
        rt.read_pfm(path)
    assert "rth_read_pfm" in str(e.value), name


def test_read_pfm_refuses_a_missing_file(rt, tmp_path):
    with pytest.raises(rt.RtError):
        rt.read_pfm(tmp_path / "none.pfm")
