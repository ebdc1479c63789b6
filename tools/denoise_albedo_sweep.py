#!/usr/bin/env python3
"""CPU only.  How the defaults of rt_denoise_albedo_params (sigma_albedo, albedo_floor) were chosen, before any device run: the numpy
restatement of the filter (tests/albedo_helpers.py) on the CPU oracle's frames — the beauty moments from its single samples, the
albedo frame from its render of the albedo description under the white-background camera with the same seed — against the oracle's
own 1024-spp mean under another seed.

    python tools/denoise_albedo_sweep.py [--reference-spp 1024]

Prints, per case, the mean squared error of the undenoised mean, of the plain filter (tests/denoise_helpers.py, defaults) and of
the guided filter at every (sigma_albedo, albedo_floor) of the sweep, as markdown rows for DESIGN.md section 5 "Albedo-guided
denoise"."""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    sys.path.insert(0, p)

CASES = [("earth_80x45_8spp", 8), ("two_perlin_spheres_80x45_8spp", 8), ("c3_cornell_box_64x64_16spp_d50", 16)]
SIGMAS = (0.05, 0.1, 0.25, 0.5, 1.0)
FLOORS = (1e-3, 1e-2, 1e-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reference-seed", type=int, default=77)
    args = ap.parse_args()
    rt = importlib.import_module("rust-tracing_amd")
    import albedo_helpers as ah
    import denoise_helpers as dh
    import oracle_lib
    import scene_cases

    print("| case | spp | undenoised | plain | " + " | ".join(f"σa {s:g}, floor {f:g}" for s in SIGMAS for f in FLOORS) + " |")
    print("|---|---|---|---|" + "---|" * (len(SIGMAS) * len(FLOORS)))
    for case, spp in CASES:
        hs = scene_cases.build(rt, case)
        shape = (hs.height, hs.width, 3)
        S, Q = dh.moments(dh.oracle_samples(rt, oracle_lib, hs, spp, args.seed), shape)
        A = oracle_lib.render(ah.AlbedoScene(rt, hs), rt.render_params(seed=args.seed, sample_end=spp)).reshape(shape)
        ref = oracle_lib.render(hs, rt.render_params(seed=args.reference_seed, sample_end=args.reference_spp)).reshape(shape) / args.reference_spp

        def mse(x):
            return float(np.mean((x - ref) ** 2))

        row = [mse(S / spp), mse(dh.denoise(S, Q, spp))]
        row += [mse(ah.denoise_albedo(S, Q, spp, A, spp, sigma_albedo=s, albedo_floor=f)) for s in SIGMAS for f in FLOORS]
        print(f"| {case} | {spp} | " + " | ".join(f"{v:.4e}" for v in row) + " |", flush=True)


if __name__ == "__main__":
    main()
