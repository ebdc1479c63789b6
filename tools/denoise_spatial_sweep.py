#!/usr/bin/env python3
"""CPU only.  How the defaults of rt_denoise_spatial_params (window_radius, spatial_below) were chosen, before any device run: the numpy
restatement of the spatial prepare (tests/spatial_denoise_helpers.py) on the CPU oracle's frames — the running mean and M2 folded from
its single samples, the albedo mean from its samples of the albedo description under the white-background camera with the same seed —
against the oracle's own 1024-spp mean under another seed.

    python tools/denoise_spatial_sweep.py [--reference-spp 1024] [--max-samples 4]

Prints, per case and sample count 1..4, the mean squared error of the unfiltered mean, of the spatial estimate at R = 1, 2, 3 (plain,
then guided), and of today's M2 filters (plain and guided; at one sample they return the input), as markdown rows for DESIGN.md
section 5 "Spatial variance"."""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    sys.path.insert(0, p)

CASES = ["c3_cornell_box_64x64_16spp_d50", "two_perlin_spheres_80x45_8spp", "earth_80x45_8spp"]
RADII = (1, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--max-samples", type=int, default=4)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reference-seed", type=int, default=77)
    args = ap.parse_args()
    rt = importlib.import_module("rust-tracing_amd")
    import albedo_helpers as ah
    import live_denoise_helpers as ldh
    import oracle_lib
    import scene_cases
    import spatial_denoise_helpers as sdh

    print("| case | samples | unfiltered | " + " | ".join(f"spatial R={r}" for r in RADII) + " | M2 filter | "
          + " | ".join(f"guided spatial R={r}" for r in RADII) + " | guided M2 filter |")
    print("|---|---|---|" + "---|" * (2 * len(RADII) + 2))
    for case in CASES:
        hs = scene_cases.build(rt, case)
        shape = (hs.height, hs.width, 3)
        n_max = args.max_samples
        colours = ldh.live_helpers.oracle_samples(rt, oracle_lib, hs, n_max, args.seed)
        albedos = ldh.live_helpers.oracle_samples(rt, oracle_lib, ah.AlbedoScene(rt, hs), n_max, args.seed)
        ref = oracle_lib.render(hs, rt.render_params(seed=args.reference_seed, sample_end=args.reference_spp)).reshape(shape) / args.reference_spp

        def mse(x):
            return float(np.mean((x - ref) ** 2))

        for n in range(1, n_max + 1):
            m, m2 = (a.reshape(shape) for a in ldh.fold_moments(colours[:n]))
            a = ldh.live_helpers.fold(albedos[:n]).reshape(shape)
            row = [mse(m)]
            row += [mse(sdh.denoise_mean_spatial(m, None, n, spatial_below=n + 1, window_radius=r)) for r in RADII]
            row += [mse(ldh.denoise_mean(m, m2, n))]
            row += [mse(sdh.denoise_albedo_mean_spatial(m, None, n, a, spatial_below=n + 1, window_radius=r)) for r in RADII]
            row += [mse(ldh.denoise_albedo_mean(m, m2, n, a))]
            print(f"| {case} | {n} | " + " | ".join(f"{v:.4e}" for v in row) + " |", flush=True)


if __name__ == "__main__":
    main()
