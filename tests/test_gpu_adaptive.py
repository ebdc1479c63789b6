"""Adaptive sampling on the GPU: the list-mode render (rt_render_pixels_device) against the dense render, the squared sums against
single-sample renders, and rt_render_adaptive against the CPU oracle at every pixel's own sample count and a numpy replay of the
rule.  Every comparison is bit for bit on the u64 view of the f64 values; sequential sums are built with Python loops."""
import subprocess

import numpy as np
import pytest

import scene_cases

pytestmark = pytest.mark.gpu

CASES = ["ragged_cornell_37x37_4spp", "cornell_smoke_64x64_16spp", "c4_final_scene_64x64_8spp_d40"]
WALKS = ["RT_WALK_REFERENCE_ORDER", "RT_WALK_OWN_TREES"]
PAD = 0xFFFFFFFF
SENTINEL = np.uint64(0x7FF8DEADBEEF0001)  # a NaN pattern no render writes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    neq = bits(got) != bits(want)
    assert not neq.any(), f"{what}: {int(neq.sum())} of {got.size} values differ (first at {int(np.flatnonzero(neq)[0])})"


def tile_order(w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    out = np.full(tx * ty * 64, PAD, dtype=np.uint32)
    for k in range(tx * ty):
        for p in range(64):
            i, j = (k % tx) * 8 + (p & 7), (k // tx) * 8 + (p >> 3)
            if i < w and j < h:
                out[k * 64 + p] = j * w + i
    return out


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


def replay(S, Q, n, rel, abs_):
    """The rule of include/rt_amd.h in numpy, elementwise f64 in the same order (numpy does not contract)."""
    m = S / float(n)
    v = (Q - S * m) / float(n - 1)
    e2 = np.maximum(np.maximum(v[:, 0], v[:, 1]), v[:, 2]) / float(n)
    L = ((m[:, 0] + m[:, 1]) + m[:, 2]) / 3.0
    tol = rel * L + abs_
    finite = np.isfinite(S).all(axis=1) & np.isfinite(Q).all(axis=1) & ~np.isnan(v).any(axis=1)
    return finite & (e2 <= tol * tol)


@pytest.mark.parametrize("walk", WALKS)
def test_adaptive_render_matches_the_oracle_at_every_pixels_own_spp(rt, oracle, gpu, walk):
    hs, ds = setup(rt, "simple_light_80x45_16spp", walk)
    w, h = hs.width, hs.height
    n_pix = w * h
    min_spp, batch, max_spp, rel, abs_ = 4, 4, 24, 0.05, 1e-3
    points = list(range(min_spp, max_spp, batch)) + [max_spp]
    # the oracle: snapshots of the running sums at each schedule point (accumulate=1), squared sums from single-sample renders
    snap, snap_q = {}, {}
    run = np.zeros(n_pix * 3)
    s_seq = np.zeros(n_pix * 3)
    q_seq = np.zeros(n_pix * 3)
    prev = 0
    for nk in points:
        oracle.render(hs, rt.render_params(seed=3, sample_begin=prev, sample_end=nk, accumulate=prev > 0), out=run)
        for s in range(prev, nk):
            c = oracle.render(hs, rt.render_params(seed=3, sample_begin=s, sample_end=s + 1))
            s_seq = s_seq + c
            q_seq = q_seq + c * c
        assert_bits(s_seq, run, f"oracle: sequential single samples against the accumulated snapshot at {nk}")
        snap[nk], snap_q[nk] = run.copy().reshape(n_pix, 3), q_seq.copy().reshape(n_pix, 3)
        prev = nk
    want_spp = np.zeros(n_pix, dtype=np.int32)
    active = np.ones(n_pix, dtype=bool)
    launches = 0
    for nk in points:
        launches += 1
        leave = active & (replay(snap[nk], snap_q[nk], nk, rel, abs_) | (nk == max_spp))
        want_spp[leave] = nk
        active &= ~leave
        if not active.any():
            break

    total, spp, sq, res = ds.render_adaptive(rt.render_params(seed=3, sample_end=max_spp), min_spp=min_spp, batch_spp=batch, rel=rel,
                                             abs=abs_)
    spp = spp.reshape(-1)
    assert (spp == want_spp).all(), f"{int((spp != want_spp).sum())} pixels' spp differ from the replay"
    assert (spp == min_spp).any() and (spp == max_spp).any(), np.unique(spp)
    total, sq = total.reshape(n_pix, 3), sq.reshape(n_pix, 3)
    for nk in points:
        sel = spp == nk
        assert_bits(total[sel], snap[nk][sel], f"sums of the pixels that stopped at {nk}")
        assert_bits(sq[sel], snap_q[nk][sel], f"squared sums of the pixels that stopped at {nk}")
    assert res["samples"] == int(spp.sum())
    assert res["launches"] == launches
    assert res["converged"] == int((spp < max_spp).sum())


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
