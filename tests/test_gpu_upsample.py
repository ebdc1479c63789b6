"""Guided upsampling on the device (rt_upsample_device) against its host mirror and the numpy restatement of include/rt_amd.h "guided
upsampling" (tests/upsample_helpers.py), bit for bit, doubles and RGBA8 bytes: every listed size at every factor with every guide set,
both kernel forms through the debug hook, the bytes asked for and not, a stream of its own, a workspace of NaN bytes, and end to end
on the Cornell box — a render under the scaled camera, upsampled under rendered guides, with the mean squared error tools/upsample_sweep.py
prints for that configuration."""
import numpy as np
import pytest

import upsample_helpers as uh

pytestmark = pytest.mark.gpu

KW = dict(sigma_edge=0.4, sigma_albedo=0.6, albedo_floor=2e-3)


@pytest.fixture(scope="module")
def cases():
    """per (w, h, F): the shared inputs (with non-finite values) and the restated result of each guide set — computed once, never written"""
    out = {}
    for w, h in uh.GPU_SHAPES:
        for F in uh.FACTORS:
            low, spp, alb, edge = uh.inputs(w, h, F, seed=w + h, special=True)
            want = {kind: uh.upsample(low, spp, (w, h), factor=F, **uh.guides_for(kind, alb, edge), **KW) for kind in uh.GUIDE_SETS}
            for a in (low, alb[0], edge[0], *want.values()):
                a.setflags(write=False)
            out[(w, h, F)] = (low, spp, alb, edge, want)
    return out


@pytest.fixture()
def form(rt):
    """forces a kernel form, and puts the built-in choice back afterwards"""
    lib = rt.amd_lib()
    yield lambda f: lib.rt_debug_set_upsample_form(f)
    lib.rt_debug_set_upsample_form(-1)


@pytest.mark.parametrize("w,h", uh.GPU_SHAPES, ids=lambda v: str(v))
def test_both_forms_give_the_mirrors_and_the_restatements_bits(rt, gpu, cases, form, w, h):
    assert form(0) == -1, "the built-in rule must have been in force"
    for F in uh.FACTORS:
        low, spp, alb, edge, want = cases[(w, h, F)]
        for kind in uh.GUIDE_SETS:
            g = uh.guides_for(kind, alb, edge)
            mirror, mirror_rgba = rt.upsample_host(low, spp, (w, h), factor=F, rgba8=True, **g, **KW)
            got = {}
            for f in (0, 1):
                form(f)
                got[f] = rt.upsample(low, spp, (w, h), factor=F, rgba8=True, **g, **KW)
                assert uh.same_bits(got[f][0], want[kind]), (F, kind, f, int((got[f][0].view(np.uint64) != want[kind].view(np.uint64)).sum()))
                assert uh.same_bits(got[f][0], mirror) and np.array_equal(got[f][1], mirror_rgba), (F, kind, f)
            assert np.array_equal(got[0][0].view(np.uint64), got[1][0].view(np.uint64)), "the two forms: the same bits, NaNs included"
            form(-1)
            assert uh.same_bits(rt.upsample(low, spp, (w, h), factor=F, **g, **KW), want[kind]), "the built-in rule, no bytes asked for"


def test_a_stream_of_its_own_and_a_workspace_of_nan_bytes(rt, gpu, cases, form):
    import torch
    w, h, F = 257, 33, 3
    low, spp, alb, edge, want = cases[(w, h, F)]
    params = rt.upsample_params(factor=F, **KW)
    d_low, d_alb, d_edge = (torch.from_numpy(np.array(a)).cuda() for a in (low, alb[0], edge[0]))
    stream = torch.cuda.Stream()
    for f in (0, 1):
        form(f)
        for kind in uh.GUIDE_SETS:
            d_ws = torch.full((rt.upsample_workspace_bytes(w, h, F),), 0xFF, dtype=torch.uint8, device="cuda")   # (all-ones doubles are NaNs)
            d_out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                rt.upsample_device(w, h, d_low.data_ptr(), spp, d_out.data_ptr(), d_ws.data_ptr(),
                                   d_albedo_sum_ptr=d_alb.data_ptr() if kind in ("albedo", "both") else 0, albedo_spp=alb[1],
                                   d_edge_sum_ptr=d_edge.data_ptr() if kind in ("edge", "both") else 0, edge_spp=edge[1],
                                   params=params, stream=stream.cuda_stream)
            stream.synchronize()
            assert uh.same_bits(d_out.cpu().numpy(), want[kind]), (f, kind)
    for d, a in ((d_low, low), (d_alb, alb[0]), (d_edge, edge[0])):
        assert np.array_equal(d.cpu().numpy().view(np.uint64), np.ascontiguousarray(a).view(np.uint64)), "the call must leave its inputs untouched"


def test_a_frame_of_many_tiles_and_a_second_call_on_a_used_workspace(rt, gpu, form):
    """1030 x 260 is 33 x 33 tiles of 32 x 8 pixels with ragged edges on both axes; the built-in rule and both forced forms give the
    restatement's bits, and so does a call on the workspace another frame's call has left behind"""
    import torch
    w, h = 1030, 260
    low, spp, alb, edge = uh.inputs(w, h, 2, seed=7)
    other = uh.inputs(w, h, 2, seed=8)[0]
    g = uh.guides_for("both", alb, edge)
    want = uh.upsample(low, spp, (w, h), **g)
    d_low, d_other, d_alb, d_edge = (torch.from_numpy(a).cuda() for a in (low, other, alb[0], edge[0]))
    d_ws = torch.zeros(rt.upsample_workspace_bytes(w, h, 2), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for f in (-1, 0, 1):
        form(f)
        for d in (d_other, d_low):
            rt.upsample_device(w, h, d.data_ptr(), spp, d_out.data_ptr(), d_ws.data_ptr(), d_albedo_sum_ptr=d_alb.data_ptr(), albedo_spp=alb[1],
                               d_edge_sum_ptr=d_edge.data_ptr(), edge_spp=edge[1], stream=stream)
        torch.cuda.synchronize()
        assert uh.same_bits(d_out.cpu().numpy(), want), f


def test_end_to_end_on_the_cornell_box(rt, gpu):
    import scene_cases
    hs = scene_cases.build(rt, "c3_cornell_box_64x64_16spp_d50")
    assert (hs.width, hs.height) == (64, 64)
    scene = rt.DeviceScene(hs, device=0)
    before = scene.render(rt.render_params(seed=3, sample_end=2))
    F, n, g = 2, 4, 4                                             # the sweep's row: 4 spp at full size = 16 spp at 32 x 32, guides at 4 spp
    cam = rt.camera_scaled(hs.camera, F)
    assert (cam.image_width, cam.image_height) == (32, 32)
    low = scene.render(rt.render_params(seed=5, sample_end=n * F * F), camera=cam)
    assert low.size == 32 * 32 * 3
    low = low.reshape(32, 32, 3)
    p = rt.render_params(seed=5, sample_end=g)
    A = rt.DeviceScene(hs, device=0, albedo=True).render(p, camera=rt.albedo_camera(hs.camera)).reshape(64, 64, 3)
    E = rt.DeviceScene(hs, device=0, surface_ids=True).render(p, camera=rt.surface_id_camera(hs.camera)).reshape(64, 64, 3)
    got, rgba = rt.upsample(low, n * F * F, (64, 64), albedo_sum=A, albedo_spp=g, edge_sum=E, edge_spp=g, rgba8=True)
    want = uh.upsample(low, n * F * F, (64, 64), albedo_sum=A, albedo_spp=g, edge_sum=E, edge_spp=g)
    assert uh.same_bits(got, want) and np.isfinite(got).all()
    assert np.array_equal(rgba, rt.tonemap_host(got, 1, rgba8=True)[1]) and len(np.unique(rgba)) > 8
    # the sweep works on the low MEANS (its low frame may have been denoised); sums with their count differ from it only in where the
    # division by the count is rounded, so its figure is asserted on the frame it describes
    swept = rt.upsample(low / (n * F * F), 1, (64, 64), albedo_sum=A, albedo_spp=g, edge_sum=E, edge_spp=g)
    ref = scene.render(rt.render_params(seed=77, sample_end=1024)).reshape(64, 64, 3) / 1024
    mse = float(np.mean((swept - ref) ** 2))
    print("cornell 64x64 F=2 albedo + ID, mse against the 1024-spp mean:", repr(mse), "plain tent:",
          repr(float(np.mean((rt.upsample(low / (n * F * F), 1, (64, 64)) - ref) ** 2))))
    assert f"{mse:.4e}" == uh.SWEEP_CORNELL_F2_BOTH, "the figure of tools/upsample_sweep.py (DESIGN.md section 5 \"Upsampling\"), to its printed digits"
    # having used the feature changes nothing for a plain render of the same scene
    after = scene.render(rt.render_params(seed=3, sample_end=2))
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
