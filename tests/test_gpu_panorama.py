"""rt_panorama_device on the GPU: the host mirror's bits at every size and face shape, on two streams, with its inputs and a canary behind
its output untouched; face choice at exact ties and the cameras' orientation on the device; and a real Cornell box end to end — six views of
one launch, each the plain render under its camera and seed, resampled to the mirror's bits, every axis looking at its own face."""
import numpy as np
import pytest

import panorama_helpers as ph

pytestmark = pytest.mark.gpu

CANARY = 8   # doubles: 64 bytes


def _device(rt, W, H, tables, faces, g, spp, stream=None):
    """one rt_panorama_device call; returns (output, the inputs as downloaded afterwards, the canary behind the output)"""
    import torch
    F = faces.shape[1]
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        d_t = torch.from_numpy(np.ascontiguousarray(tables)).cuda()
        d_f = torch.from_numpy(np.ascontiguousarray(faces)).cuda()
        d_o = torch.full((3 * W * H + CANARY,), -7.5, dtype=torch.float64, device="cuda")
        rt.panorama_device(W, H, d_t.data_ptr(), d_f.data_ptr(), F, g, spp, d_o.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()
        out = d_o.cpu().numpy()
        return out[:3 * W * H].reshape(H, W, 3), d_t.cpu().numpy(), d_f.cpu().numpy(), out[3 * W * H:]


@pytest.mark.parametrize("spp", (3, 1))
@pytest.mark.parametrize("F,g", ph.FACES)
@pytest.mark.parametrize("W,H", ph.SIZES)
def test_the_device_gives_the_mirrors_bits_and_touches_nothing_else(rt, gpu, W, H, F, g, spp):
    import torch
    faces = ph.random_faces(F, 100 * F + g, spp)
    t = rt.panorama_tables(W, H)
    want = rt.panorama_host(W, H, faces, g, spp, tables=t)
    for stream in (None, torch.cuda.Stream()):
        got, t_after, f_after, canary = _device(rt, W, H, t, faces, g, spp, stream)
        assert np.array_equal(ph.bits(got), ph.bits(want))
        assert np.array_equal(ph.bits(t_after), ph.bits(t)) and np.array_equal(ph.bits(f_after), ph.bits(faces))
        assert np.array_equal(canary, np.full(CANARY, -7.5))


@pytest.mark.parametrize("F,g", ph.FACES)
def test_exact_ties_choose_the_face_the_header_prescribes(rt, gpu, F, g):
    t, W, H, want = ph.tie_tables()
    got = rt.panorama(W, H, ph.index_faces(F), g, 1, tables=t)
    assert np.array_equal(got, np.repeat(want[..., None].astype(np.float64), 3, axis=2))


@pytest.mark.parametrize("F,g", ((10, 1), (12, 2)))
def test_cameras_and_resampler_agree_on_every_faces_orientation(rt, gpu, F, g):
    W, H = 64, 32
    t = rt.panorama_tables(W, H)
    faces = ph.direction_faces(F, g)
    got = rt.panorama(W, H, faces, g, 1, tables=t)
    err = float(np.max(np.abs(got - ph.own_direction(t, W, H))))
    print(F, g, err)
    assert err <= 1e-12
    assert np.array_equal(ph.bits(got), ph.bits(rt.panorama_host(W, H, faces, g, 1, tables=t)))


CENTER = (430.0, 450.0, 120.0)   # inside the Cornell box, above both blocks and off the lamp: every axis meets one flat surface (-Z: the open front)
SPP, SEED = 4, 11


@pytest.fixture(scope="module")
def box(rt):
    hs = rt.HostScene(6, scene_seed=1, width=32, aspect=1.0, spp=SPP, depth=8)   # cornell_box
    return hs, rt.DeviceScene(hs, surface_ids=True)


def test_a_cornell_box_end_to_end(rt, gpu, box):
    import torch
    hs, ds = box
    W, H, F, g = 64, 32, 18, 1
    pano = ds.render_panorama(W, center=CENTER, spp=SPP, seed=SEED)
    assert pano.shape == (H, W, 3)
    views = ds.panorama_views(F, g, CENTER, SEED)
    stack = ds.render_views(rt.render_params(sample_end=SPP), views)
    assert stack.shape == (6, F, F, 3)
    assert np.array_equal(ph.bits(pano), ph.bits(rt.panorama_host(W, H, stack, g, SPP)))
    # the views contract on the new cameras: view f is the plain render under camera f and seed SEED + f
    for f in range(6):
        d_one = torch.zeros((F, F, 3), dtype=torch.float64, device="cuda")
        ds.render_device(rt.render_params(seed=SEED + f, sample_end=SPP), d_one.data_ptr(), torch.cuda.current_stream().cuda_stream, camera=views[f].camera)
        torch.cuda.synchronize()
        assert np.array_equal(ph.bits(d_one.cpu().numpy()), ph.bits(stack[f])), f
    # every axis looks at the centre of its own face: columns 3W/4, W/4, any, any, 0 | W - 1, W/2 on the equator, and the two poles
    mid = slice(F // 2 - 1, F // 2 + 1)
    centre = [stack[f, mid, mid].reshape(4, 3) * (1.0 / SPP) for f in range(6)]
    for f in range(6):
        assert (centre[f] == centre[f][0]).all(), f"face {f}: the four centre texels must show one surface"
    assert len({tuple(c[0]) for c in centre}) >= 5, "the walls, floor and ceiling carry surface IDs of their own"
    rows, cols = (H // 2 - 1, H // 2), lambda k: (k - 1, k % W)
    near = {0: (rows, cols(3 * W // 4)), 1: (rows, cols(W // 4)), 2: ((0,), range(W)), 3: ((H - 1,), range(W)), 4: (rows, cols(0)), 5: (rows, cols(W // 2))}
    for f, (jj, ii) in near.items():
        for j in jj:
            for i in ii:
                assert np.array_equal(pano[j, i], centre[f][0]), (f, j, i)
