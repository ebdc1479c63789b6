"""Adaptive sampling on the GPU: the list-mode render (rt_render_pixels_device) against the dense render, the squared sums against
single-sample renders, and rt_render_adaptive against the CPU oracle at every pixel's own sample count and a numpy replay of the
rule.  Every comparison is bit for bit on the u64 view of the f64 values; sequential sums are built with Python loops."""
import subprocess

import numpy as np
import pytest

import scene_cases
from adaptive_helpers import PAD, SENTINEL, assert_bits, bits, check_adaptive_against_oracle, tile_order

pytestmark = pytest.mark.gpu

CASES = ["ragged_cornell_37x37_4spp", "cornell_smoke_64x64_16spp", "c4_final_scene_64x64_8spp_d40"]
WALKS = ["RT_WALK_REFERENCE_ORDER", "RT_WALK_OWN_TREES"]


def setup(rt, case, walk, **kw):
    hs = scene_cases.build(rt, case, **kw)
    return hs, rt.DeviceScene(hs, walk=getattr(rt, walk))


def dense(rt, ds, hs, b, e, seed=3):
    import torch
    d = torch.zeros(hs.width * hs.height * 3, dtype=torch.float64, device="cuda")
    ds.render_device(rt.render_params(seed=seed, sample_begin=b, sample_end=e), d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def listed(rt, ds, pixels, b, e, s0, q0=None, accumulate=False, seed=3):
    """rt_render_pixels_device onto copies of s0 (and q0); returns the sums (and squared sums) as numpy."""
    import torch
    lst = torch.from_numpy(np.ascontiguousarray(pixels, dtype=np.uint32).view(np.int32)).cuda()
    s = torch.from_numpy(np.array(s0, dtype=np.float64)).cuda()
    q = torch.from_numpy(np.array(q0, dtype=np.float64)).cuda() if q0 is not None else None
    ds.render_pixels_device(rt.render_params(seed=seed, sample_begin=b, sample_end=e, accumulate=accumulate), lst.data_ptr(), len(pixels),
                            s.data_ptr(), q.data_ptr() if q is not None else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return s.cpu().numpy(), (q.cpu().numpy() if q is not None else None)


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("case", CASES)
def test_full_list_in_tile_order_equals_the_dense_frame(rt, gpu, case, walk):
    hs, ds = setup(rt, case, walk)
    n = hs.camera.samples_per_pixel
    want = dense(rt, ds, hs, 0, n)
    zeros = np.zeros_like(want)
    got, _ = listed(rt, ds, tile_order(hs.width, hs.height), 0, n, zeros, zeros)
    assert_bits(got, want, f"{case} full list")


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("case", CASES)
def test_a_shuffled_subset_with_padding_writes_only_its_pixels(rt, gpu, case, walk):
    hs, ds = setup(rt, case, walk)
    n_pix, n = hs.width * hs.height, hs.camera.samples_per_pixel
    want = dense(rt, ds, hs, 0, n).reshape(n_pix, 3)
    g = np.random.default_rng(7)
    chosen = g.choice(n_pix, size=n_pix // 3, replace=False).astype(np.uint32)
    g.shuffle(chosen)
    pixels = np.insert(chosen, g.integers(0, chosen.size, 11), PAD)  # padding entries anywhere in the list
    init = np.full((n_pix, 3), SENTINEL, dtype=np.uint64).view(np.float64)
    got, sq = listed(rt, ds, pixels, 0, n, init, init)
    got, sq = got.reshape(n_pix, 3), sq.reshape(n_pix, 3)
    mask = np.zeros(n_pix, dtype=bool)
    mask[chosen] = True
    assert_bits(got[mask], want[mask], f"{case}: listed pixels")
    assert (bits(got[~mask]) == SENTINEL).all() and (bits(sq[~mask]) == SENTINEL).all(), f"{case}: an unlisted pixel was written"
    assert (bits(sq[mask]) != SENTINEL).all()


@pytest.mark.parametrize("case", ["ragged_cornell_37x37_4spp", "c4_final_scene_64x64_8spp_d40"])
def test_squared_sums_equal_the_sequential_sum_of_single_sample_squares(rt, gpu, case):
    hs, ds = setup(rt, case, "RT_WALK_OWN_TREES")
    n = 6
    s_want = np.zeros(hs.width * hs.height * 3)
    q_want = np.zeros_like(s_want)
    for s in range(n):  # sequential: ((c0 + c1) + c2) ..., each c * c rounded before it is added
        c = dense(rt, ds, hs, s, s + 1)
        s_want = s_want + c
        q_want = q_want + c * c
    zeros = np.zeros_like(s_want)
    got, sq = listed(rt, ds, tile_order(hs.width, hs.height), 0, n, zeros, zeros)
    assert_bits(got, s_want, "sums")
    assert_bits(sq, q_want, "squared sums")


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("case", CASES)
def test_a_list_render_continued_with_accumulate_equals_one_render(rt, gpu, case, walk):
    hs, ds = setup(rt, case, walk)
    lst = tile_order(hs.width, hs.height)
    zeros = np.zeros(hs.width * hs.height * 3)
    whole, whole_sq = listed(rt, ds, lst, 0, 7, zeros, zeros)
    first, first_sq = listed(rt, ds, lst, 0, 3, zeros, zeros)
    both, both_sq = listed(rt, ds, lst, 3, 7, first, first_sq, accumulate=True)
    assert_bits(both, whole, "sums")
    assert_bits(both_sq, whole_sq, "squared sums")


@pytest.mark.parametrize("case", ["ragged_cornell_37x37_4spp", "c4_final_scene_64x64_8spp_d40"])
def test_min_spp_equal_to_max_spp_is_the_uniform_render(rt, gpu, case):
    import torch
    hs, ds = setup(rt, case, "RT_WALK_OWN_TREES")
    w, h, n = hs.width, hs.height, 6
    want = dense(rt, ds, hs, 0, n)
    total, spp, sq, res = ds.render_adaptive(rt.render_params(seed=3, sample_end=n), min_spp=n, batch_spp=4, rel=0.5, abs=1.0)
    assert (spp == n).all()
    assert_bits(total.reshape(-1), want, "sums")
    assert res == {"samples": w * h * n, "launches": 1, "converged": 0}
    d_sum = torch.from_numpy(total.reshape(-1)).cuda()
    d_spp = torch.from_numpy(spp.reshape(-1)).cuda()
    a = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    b = torch.zeros_like(a)
    stream = torch.cuda.current_stream().cuda_stream
    rt.resolve_rgb8_spp_device(w, h, d_sum.data_ptr(), d_spp.data_ptr(), a.data_ptr(), stream)
    rt.resolve_rgb8_device(w, h, n, d_sum.data_ptr(), b.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("walk", WALKS)
def test_adaptive_render_matches_the_oracle_at_every_pixels_own_spp(rt, oracle, gpu, walk):
    """(the oracle's snapshots, the numpy replay of the rule and the assertions: adaptive_helpers.check_adaptive_against_oracle, shared
    with the full-frame cases of tests/test_gpu_full_size.py)"""
    hs, ds = setup(rt, "simple_light_80x45_16spp", walk)
    check_adaptive_against_oracle(rt, oracle, hs, ds, min_spp=4, batch=4, max_spp=24, rel=0.05, abs_=1e-3)


def test_per_pixel_spp_resolve_equals_the_uniform_resolve_per_group(rt, gpu):
    import torch
    hs, ds = setup(rt, "c3_cornell_box_64x64_16spp_d50", "RT_WALK_OWN_TREES")
    w, h = hs.width, hs.height
    a = rt.adaptive_params(min_spp=4, batch_spp=3, rel_threshold=0.1, abs_threshold=0.01)
    d_sum = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    d_spp = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    import ctypes as C
    res = rt.AdaptiveResult()
    params = rt.render_params(seed=3, sample_end=16)
    rc = rt.amd_lib().rt_render_adaptive_device(ds._handle, C.byref(hs.camera), C.byref(params), C.byref(a), C.c_void_p(d_sum.data_ptr()),
                                                C.c_void_p(d_spp.data_ptr()), None, C.c_void_p(stream), C.byref(res))
    assert rc == 0, rt.amd_lib().rt_last_error()
    rt.resolve_rgb8_spp_device(w, h, d_sum.data_ptr(), d_spp.data_ptr(), d_rgb.data_ptr(), stream)
    torch.cuda.synchronize()
    # the device form and the host form agree
    total, spp_h, _, res_h = ds.render_adaptive(params, min_spp=4, batch_spp=3, rel=0.1, abs=0.01)
    assert_bits(d_sum.cpu().numpy(), total.reshape(-1), "device against host form")
    assert (d_spp.cpu().numpy() == spp_h.reshape(-1)).all() and res.as_dict() == res_h
    spp = d_spp.cpu().numpy()
    got = d_rgb.cpu().numpy().reshape(w * h, 3)
    sums = d_sum.reshape(w * h, 3)
    groups = np.unique(spp)
    assert groups.size >= 2, groups
    for n in groups:
        idx = torch.from_numpy(np.flatnonzero(spp == n)).cuda()
        part = sums[idx].contiguous().reshape(-1)
        out = torch.zeros(part.numel(), dtype=torch.uint8, device="cuda")
        rt.resolve_rgb8_values_device(part.numel(), int(n), part.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(-1, 3), got[spp == n]), f"pixels at spp {n}"


def test_rtrace_adaptive_at_min_spp_equal_to_spp_writes_the_plain_png(rt, gpu, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    args = ["-s", "6", "--width", "48", "--spp", "12", "--depth", "8", "--seed", "5", "--scene-seed", "1"]
    r = subprocess.run([str(exe), *args, "-o", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), *args, "--adaptive", "0.05", "--min-spp", "12", "--batch-spp", "4", "-o", str(tmp_path / "adaptive")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Adaptive:")]
    assert line and "mean 12.00 spp, min 12, max 12, 1 launches" in line[0], r.stdout
    assert (tmp_path / "plain.png").read_bytes() == (tmp_path / "adaptive.png").read_bytes()
    # a real threshold: the mean drops below the maximum
    r = subprocess.run([str(exe), *args, "--adaptive", "0.2", "--adaptive-abs", "0.05", "--min-spp", "4", "-o", str(tmp_path / "a2")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "a2.png").exists() and "Adaptive:" in r.stdout
