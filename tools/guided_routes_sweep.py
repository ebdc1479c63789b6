#!/usr/bin/env python3
"""CPU only.  What the edge guide does to the means, spatial-variance and views routes of the denoiser, before any device run: the numpy
restatements (tests/guided_routes_helpers.py and the ones it is built from) on the CPU oracle's frames of the Cornell box at 64 x 64 —
the running mean and M2 folded from its single samples, the surface-ID frame of means from its samples of the surface-ID description
under the black-background camera (min(n, 16) samples, the same seed) — against the oracle's own 1024-spp mean under seed 77.

    python tools/guided_routes_sweep.py [--out FILE] [--reference-spp 1024] [--seed 5]

Prints the mean squared error of: the undenoised mean; the plain means form (at one sample it returns its input) and the edge-guided
one; both through the spatial route at one sample (R = 1, 2, 3); and, on a 3-view orbit of 4 samples per view (view k under seed + k),
the plain and the edge-guided views form per view — as markdown rows for DESIGN.md section 5 "Edge guide on every route"."""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    sys.path.insert(0, p)

CASE = "c3_cornell_box_64x64_16spp_d50"
SAMPLES = (1, 2, 4, 16)
RADII = (1, 2, 3)
GUIDE_SPP = 16


class WithCamera:
    """a scene's description under another camera: quacks like rt.HostScene for the oracle"""

    def __init__(self, scene, camera):
        self.scene, self.desc, self.camera = scene, scene.desc, camera

    width = property(lambda self: self.camera.image_width)
    height = property(lambda self: self.camera.image_height)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reference-seed", type=int, default=77)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--views-spp", type=int, default=4)
    args = ap.parse_args()
    rt = importlib.import_module("rust-tracing_amd")
    import denoise_helpers as dh
    import guided_helpers as gh
    import guided_routes_helpers as grh
    import live_denoise_helpers as ldh
    import oracle_lib
    import scene_cases
    import spatial_denoise_helpers as sdh
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    hs = scene_cases.build(rt, CASE)
    shape = (hs.height, hs.width, 3)
    ids = gh.SurfaceIdScene(rt, hs)
    colours = ldh.live_helpers.oracle_samples(rt, oracle_lib, hs, max(SAMPLES), args.seed)
    guides = ldh.live_helpers.oracle_samples(rt, oracle_lib, ids, GUIDE_SPP, args.seed)
    ref = oracle_lib.render(hs, rt.render_params(seed=args.reference_seed, sample_end=args.reference_spp)).reshape(shape) / args.reference_spp

    def mse(x, r=ref):
        return float(np.mean((x - r) ** 2))

    log(f"tools/guided_routes_sweep.py: {CASE}, samples under seed {args.seed}, against the oracle's {args.reference_spp}-spp mean under seed "
        f"{args.reference_seed}; default filter parameters (K = 4, sigma_edge = 0.5); mean squared errors")
    log("")
    log("| samples | undenoised | means, plain | means, edge-guided | " + " | ".join(f"spatial R={r}, plain | spatial R={r}, edge-guided" for r in RADII) + " |")
    log("|---|---|---|---|" + "---|---|" * len(RADII))
    for n in SAMPLES:
        m, m2 = (a.reshape(shape) for a in ldh.fold_moments(colours[:n]))
        e = ldh.live_helpers.fold(guides[:min(n, GUIDE_SPP)]).reshape(shape)
        row = [f"{mse(m):.4e}", f"{mse(ldh.denoise_mean(m, m2, n)):.4e}", f"{mse(grh.denoise_guided_mean(m, m2, n, e)):.4e}"]
        for r in RADII:
            if n == 1:
                row += [f"{mse(sdh.denoise_mean_spatial(m, None, 1, window_radius=r)):.4e}",
                        f"{mse(grh.denoise_guided_mean_spatial(m, None, 1, e, window_radius=r)):.4e}"]
            else:
                row += ["(means form)", "(means form)"]
        log(f"| {n} | " + " | ".join(row) + " |")
    log("")
    log(f"| view of {args.views} ({args.views_spp} spp, seed + k) | undenoised | views, plain | views, edge-guided |")
    log("|---|---|---|---|")
    views = rt.orbit_views(hs, args.views, args.seed)
    spp = args.views_spp
    for k in range(args.views):
        cam = views[k].camera
        seed = int(views[k].seed)
        scene, id_scene = WithCamera(hs, cam), WithCamera(ids, rt.surface_id_camera(cam))
        S, Q = dh.moments(ldh.live_helpers.oracle_samples(rt, oracle_lib, scene, spp, seed), shape)
        E = oracle_lib.render(id_scene, rt.render_params(seed=seed, sample_end=spp)).reshape(shape)
        r = oracle_lib.render(scene, rt.render_params(seed=args.reference_seed, sample_end=args.reference_spp)).reshape(shape) / args.reference_spp
        log(f"| {k} | {mse(S / spp, r):.4e} | {mse(dh.denoise(S, Q, spp), r):.4e} | {mse(grh.denoise_guided_views(S[None], Q[None], spp, E[None], spp)[0], r):.4e} |")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
