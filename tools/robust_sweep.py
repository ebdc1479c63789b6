#!/usr/bin/env python3
"""CPU (the plain-C oracle and the host mirror rth_robust; no GPU).  What the robust-frame estimator buys: on the Cornell box,
simple_light and final_scene at a small frame and total budgets of 16 and 64 samples per pixel, the plain mean of all samples against
rt_robust's modes over K = 4, 8, 16 blocks (block k: the camera under seed + k, budget / K samples — what `rtrace --robust K` renders),
measured against a high-spp oracle frame of the same scene:

    relMSE   mean over the values of (x - ref)^2 / (ref^2 + 1e-2)
    bias     mean over the values of (x - ref) / (mean of ref): the signed error, as a fraction of the frame's mean radiance
             (a median darkens skewed pixels: negative)

each averaged over --trials seeds, and the same again with the means-form a-trous filter (the numpy restatement of
rt_denoise_mean_device, samples = K) behind both estimators — the plain mean then enters as RT_ROBUST_MEAN with its own M2.

    python tools/robust_sweep.py [--width 48] [--ref-spp 4096] [--trials 4]

Prints the tables (markdown, for DESIGN.md section 5 "Robust frames")."""
import argparse
import importlib
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

SCENES = ((6, "cornell_box", 1.0), (5, "simple_light", 1.5), (8, "final_scene", 1.0))
KS = (4, 8, 16)
GAINS = (0.5, 1.0, 2.0, 4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=48)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--trials", type=int, default=4)
    ap.add_argument("--depth", type=int, default=16)
    args = ap.parse_args()
    import numpy as np
    import live_denoise_helpers as ldh
    import oracle_lib
    from source_hash import source_hash
    rt = importlib.import_module("rust-tracing_amd")
    modes = [("mean", dict(mode="mean")), ("trim 1", dict(mode="trim", trim=1)), ("median", dict(mode="median"))] + \
            [(f"gini {g:g}", dict(mode="gini", gain=g)) for g in GAINS]

    def errors(x, ref):
        d = x - ref
        return float(np.mean(d * d / (ref * ref + 1e-2))), float(np.mean(d) / np.mean(ref))

    print(f"sources {source_hash()}; width {args.width}, depth {args.depth}, reference {args.ref_spp} spp (oracle), {args.trials} trials; "
          "relMSE / bias, unfiltered || behind the means-form filter (samples = K)")
    for scene, name, aspect in SCENES:
        hs = rt.HostScene(scene, scene_seed=1, width=args.width, aspect=aspect, spp=16, depth=args.depth)
        w, h = hs.width, hs.height
        ref = oracle_lib.render(hs, rt.render_params(seed=987654321, sample_end=args.ref_spp)).reshape(h, w, 3) * (1.0 / args.ref_spp)
        for budget in (16, 64):
            acc = {}
            for trial in range(args.trials):
                seed = 1000 * (trial + 1)
                plain = oracle_lib.render(hs, rt.render_params(seed=seed, sample_end=budget)).reshape(h, w, 3) * (1.0 / budget)
                acc.setdefault(("plain", 0), []).append(errors(plain, ref) + (float("nan"), float("nan")))
                for K in KS:
                    stack = np.stack([oracle_lib.render(hs, rt.render_params(seed=seed + k, sample_end=budget // K)).reshape(h, w, 3) for k in range(K)])
                    for label, kw in modes:
                        mean, m2 = rt.robust_host(stack, budget // K, m2=True, **kw)
                        acc.setdefault((label, K), []).append(errors(mean, ref) + errors(ldh.denoise_mean(mean, m2, K), ref))
            print(f"\n{name} {w} x {h}, {budget} spp in total")
            print("| estimator | " + " | ".join(f"K = {K}" for K in KS) + " |")
            print("|---|" + "---|" * len(KS))
            e = np.mean(acc[("plain", 0)], axis=0)
            print(f"| the plain mean of all {budget} samples | " + " | ".join([f"{e[0]:.4f} / {e[1]:+.3f}"] * len(KS)) + " |")
            for label, _ in modes:
                cells = []
                for K in KS:
                    e = np.mean(acc[(label, K)], axis=0)
                    cells.append(f"{e[0]:.4f} / {e[1]:+.3f} \\|\\| {e[2]:.4f} / {e[3]:+.3f}")
                print(f"| {label} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
