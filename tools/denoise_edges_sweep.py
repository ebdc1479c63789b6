#!/usr/bin/env python3
"""CPU only.  What an edge guide is worth and how the default of rt_denoise_guided_params.sigma_edge was chosen, before any device
run: the numpy restatement of the filter (tests/guided_helpers.py) on the CPU oracle's frames — the beauty moments from its single
samples, the surface-ID and the albedo frames from its renders of the transformed descriptions (black / white background) with the
same seed — against the oracle's own 1024-spp mean under another seed.  The frames and the truth are those of
tools/denoise_albedo_sweep.py, with cornell_smoke added.

    python tools/denoise_edges_sweep.py [--reference-spp 1024]

Prints, per case, the mean squared error of the undenoised mean, of the plain filter, of the albedo-guided filter (defaults) and, at
every sigma_edge of the sweep, of the three uses of the edge guide: the ID frame alone, the albedo frame itself as the edge guide (the
albedo stop without the demodulation), and the ID frame beside the demodulating albedo guide — as markdown rows for DESIGN.md section
5 "Edge-guided denoise"."""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    sys.path.insert(0, p)

CASES = [("earth_80x45_8spp", 8), ("two_perlin_spheres_80x45_8spp", 8), ("c3_cornell_box_64x64_16spp_d50", 16), ("cornell_smoke_64x64_16spp", 16)]
SIGMAS = (0.125, 0.25, 0.5, 0.75, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reference-seed", type=int, default=77)
    args = ap.parse_args()
    rt = importlib.import_module("rust-tracing_amd")
    import albedo_helpers as ah
    import denoise_helpers as dh
    import guided_helpers as gh
    import oracle_lib
    import scene_cases

    print("| case | spp | σe | undenoised | plain | albedo-guided | edges: ID frame | edges: albedo frame | albedo + ID edges |")
    print("|---|---|---|---|---|---|---|---|---|")
    for case, spp in CASES:
        hs = scene_cases.build(rt, case)
        shape = (hs.height, hs.width, 3)
        p = rt.render_params(seed=args.seed, sample_end=spp)
        S, Q = dh.moments(dh.oracle_samples(rt, oracle_lib, hs, spp, args.seed), shape)
        A = oracle_lib.render(ah.AlbedoScene(rt, hs), p).reshape(shape)
        E = oracle_lib.render(gh.SurfaceIdScene(rt, hs), p).reshape(shape)
        ref = oracle_lib.render(hs, rt.render_params(seed=args.reference_seed, sample_end=args.reference_spp)).reshape(shape) / args.reference_spp

        def mse(x):
            return float(np.mean((x - ref) ** 2))

        fixed = [mse(S / spp), mse(dh.denoise(S, Q, spp)), mse(ah.denoise_albedo(S, Q, spp, A, spp))]
        for s in SIGMAS:
            row = fixed + [mse(gh.denoise_guided(S, Q, spp, E, spp, sigma_edge=s)), mse(gh.denoise_guided(S, Q, spp, A, spp, sigma_edge=s)),
                           mse(gh.denoise_guided(S, Q, spp, E, spp, A, spp, sigma_edge=s))]
            print(f"| {case} | {spp} | {s:g} | " + " | ".join(f"{v:.4e}" for v in row) + " |", flush=True)


if __name__ == "__main__":
    main()
