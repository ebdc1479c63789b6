#!/usr/bin/env python3
"""CPU only.  What tracing a smaller frame and upsampling it is worth at an equal sample budget, and how the defaults of
rt_upsample_params.sigma_edge and sigma_albedo were chosen, before any device run: the numpy restatement of the upsampler
(tests/upsample_helpers.py) and of the plain denoiser (tests/denoise_helpers.py) on the CPU oracle's frames, against the oracle's own
1024-spp mean under another seed.

    python tools/upsample_sweep.py [--reference-spp 1024] [--full-spp 4] [--guide-spp 4]

Per scene (the Cornell box and the earth, 64 x 64) and factor F = 2, 4: the full-size frame at --full-spp samples per pixel, and the
low frame — rendered under rt_camera_scaled at full-spp * F^2 samples per pixel, the same number of paths — brought to full size by
the plain tent, with the surface-ID guide, and with the albedo and the ID guide (both first-hit renders at --guide-spp), each from the
raw low means and from the low frame denoised at its own size (the plain filter, defaults).  Prints the mean squared errors as markdown
rows for DESIGN.md section 5 "Upsampling": first at the default sigmas, then the sweep of each sigma with the other at its default."""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    sys.path.insert(0, p)

# (label, scene case, overrides): the earth case is built at 64 x 64, not at its own 80 x 45
CASES = [("cornell_box 64x64 d50", "c3_cornell_box_64x64_16spp_d50", {}), ("earth 64x64 d8", "earth_80x45_8spp", dict(width=64, aspect=1.0))]
FACTORS = (2, 4)
SIGMAS = (0.125, 0.25, 0.5, 1.0, 2.0)


def frames(rt, oracle_lib, hs, camera, spp, seed):
    """(S, Q) of `spp` single samples under `camera`, as (h, w, 3)"""
    import denoise_helpers as dh
    shape = (camera.image_height, camera.image_width, 3)
    samples = [oracle_lib.render(hs, rt.render_params(seed=seed, sample_begin=s, sample_end=s + 1), camera=camera) for s in range(spp)]
    return dh.moments(samples, shape)


def inputs(rt, oracle_lib, hs, F, full_spp, guide_spp, seed):
    """the low moments at full_spp * F^2 samples under the scaled camera, and the full-size albedo and ID sums at guide_spp"""
    import albedo_helpers as ah
    import guided_helpers as gh
    shape = (hs.height, hs.width, 3)
    low_spp = full_spp * F * F
    S, Q = frames(rt, oracle_lib, hs, rt.camera_scaled(hs.camera, F), low_spp, seed)
    p = rt.render_params(seed=seed, sample_end=guide_spp)
    A = oracle_lib.render(ah.AlbedoScene(rt, hs), p).reshape(shape)
    E = oracle_lib.render(gh.SurfaceIdScene(rt, hs), p).reshape(shape)
    return S, Q, low_spp, A, E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--full-spp", type=int, default=4)
    ap.add_argument("--guide-spp", type=int, default=4)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reference-seed", type=int, default=77)
    args = ap.parse_args()
    rt = importlib.import_module("rust-tracing_amd")
    import denoise_helpers as dh
    import oracle_lib
    import scene_cases
    import upsample_helpers as uh

    head = "| scene | F | low spp | denoised first | (a) full size | (b) plain tent | (c) ID guide | (d) albedo + ID |"
    rows, sweep = [], []
    for case, name, overrides in CASES:
        hs = scene_cases.build(rt, name, **overrides)
        w, h, n, g = hs.width, hs.height, args.full_spp, args.guide_spp
        assert (w, h) == (64, 64), "the labels say 64 x 64"
        shape = (h, w, 3)
        ref = oracle_lib.render(hs, rt.render_params(seed=args.reference_seed, sample_end=args.reference_spp)).reshape(shape) / args.reference_spp

        def mse(x):
            return float(np.mean((x - ref) ** 2))

        Sf, Qf = frames(rt, oracle_lib, hs, hs.camera, n, args.seed)
        full = {"no": mse(Sf / n), "yes": mse(dh.denoise(Sf, Qf, n))}
        for F in FACTORS:
            S, Q, low_spp, A, E = inputs(rt, oracle_lib, hs, F, n, g, args.seed)
            lows = {"no": S / low_spp, "yes": dh.denoise(S, Q, low_spp)}
            for first, low in lows.items():
                up = lambda **kw: mse(uh.upsample(low, 1, (w, h), factor=F, **kw))   # noqa: E731
                rows.append(f"| {case} | {F} | {low_spp} | {first} | {full[first]:.4e} | {up():.4e} | {up(edge_sum=E, edge_spp=g):.4e} | "
                            f"{up(edge_sum=E, edge_spp=g, albedo_sum=A, albedo_spp=g):.4e} |")
                for s in SIGMAS:
                    sweep.append(f"| {case} | {F} | {first} | {s:g} | {up(edge_sum=E, edge_spp=g, sigma_edge=s):.4e} | "
                                 f"{up(edge_sum=E, edge_spp=g, albedo_sum=A, albedo_spp=g, sigma_edge=s):.4e} | "
                                 f"{up(edge_sum=E, edge_spp=g, albedo_sum=A, albedo_spp=g, sigma_albedo=s):.4e} |")
            print(f"# {case} F={F} done", file=sys.stderr, flush=True)
    print(head)
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))
    print()
    print("| scene | F | denoised first | σ | (c) at σe = σ | (d) at σe = σ | (d) at σa = σ |")
    print("|---|---|---|---|---|---|---|")
    print("\n".join(sweep))


if __name__ == "__main__":
    main()
