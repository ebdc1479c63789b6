#!/usr/bin/env python3
"""MI355X.  What the robust-frame combiner costs: milliseconds per rt_robust_device call (HIP events, 3 warm-up calls, the median and
the minimum of --repeats calls) on stacks of K = 4, 8, 16, 32 blocks at 1200 x 800 and at 256 x 256, with and without the M2 output, for
every kernel form that can run that K (rt_debug_set_robust_form: 4, 8, 16 or 32 register slots; the built-in rule is the smallest that
fits), and beside them, from the same session,

    rt_denoise_device, plain, K = 4       on one frame of that size
    rt_tonemap_device, ACES, RGBA8        a streaming pass over one frame
    rt_bloom_device, K = 5                nine to eleven streaming passes over one frame: the rate a bandwidth-bound kernel reaches here
    rt_render_views_device                the K sub-frames themselves, scene 5 (simple_light) at 16 spp in total, 16 / K per block (K = 32: 1 per block)

    python tools/robust_speed.py [--repeats 20]

The stack is synthetic (block sums around a common level, a firefly in one block of every sixth value: the combiner reads no scene).
Beside each time stand the bytes the launch must move at the least — K frames read, one or two written: (K + 1 or 2) * 24 * w * h — and
that figure over the median as GB/s.  Prints the tables (markdown, for DESIGN.md section 5 "Robust frames") and one JSON line."""
import argparse
import importlib
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from source_hash import source_hash  # noqa: E402
from bloom_speed import builtin_fused_max, least_bytes as bloom_least_bytes  # noqa: E402

FORMS = (4, 8, 16, 32)


def timed(fn, repeats, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("rust-tracing_amd")
    lib = rt.amd_lib()
    stream = torch.cuda.current_stream().cuda_stream
    lib.rt_debug_set_robust_form(0)
    rows = []
    for w, h in ((1200, 800), (256, 256)):
        rng = np.random.default_rng(1)
        n = w * h * 3
        level = 10.0 ** rng.uniform(-3.0, 2.0, size=n)
        full = level[None] * rng.lognormal(0.0, 0.4, size=(32, n))
        hot = np.flatnonzero(rng.random(n) < 1.0 / 6.0)
        full[rng.integers(0, 32, size=hot.size), hot] *= 10.0 ** rng.uniform(1.7, 3.7, size=hot.size)
        d_full = torch.from_numpy(full).cuda()
        d_out = torch.zeros((2, h, w, 3), dtype=torch.float64, device="cuda")
        d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        d_dws = torch.zeros(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        d_sum = d_full[0] * 4.0
        d_sq = d_full[0] * d_full[0] * 6.0
        aces, dn = rt.tonemap_params(op="aces"), rt.denoise_params(iterations=4)
        hs = rt.HostScene(5, scene_seed=1, width=w, aspect=w / h, spp=16, depth=50)
        assert (hs.width, hs.height) == (w, h)
        ds = rt.DeviceScene(hs, device=0)
        d_views = torch.zeros((32, h, w, 3), dtype=torch.float64, device="cuda")
        row = dict(width=w, height=h, robust=[])

        def combine(K, m2):
            rt.robust_device(w, h, K, d_full.data_ptr(), 4, d_out[0].data_ptr(), d_m2_out_ptr=d_out[1].data_ptr() if m2 else 0, stream=stream)

        for K in FORMS:
            reference = None
            for form in (f for f in FORMS if f >= K):
                lib.rt_debug_set_robust_form(form)
                for m2 in (False, True):
                    med, lo = timed(lambda: combine(K, m2), args.repeats, torch)
                    b = (K + (2 if m2 else 1)) * 24 * w * h
                    row["robust"].append(dict(blocks=K, form=form, builtin=form == K, m2=m2, ms=round(med, 4), min_ms=round(lo, 4), bytes=b,
                                              gb_per_s=round(b / med / 1e6, 1)))
                torch.cuda.synchronize()
                got = d_out.cpu().numpy()
                if reference is None:
                    reference = got
                assert np.array_equal(got.view(np.uint64), reference.view(np.uint64)), "the forms must give the same bits"
            lib.rt_debug_set_robust_form(0)
            views = [(hs.camera, 1 + k) for k in range(K)]
            params = rt.render_params(sample_end=max(1, 16 // K))   # (K = 32 has no 16-spp split: one sample per block, 32 in total)
            med, lo = timed(lambda: ds.render_views_device(params, views, d_views.data_ptr(), stream), max(3, args.repeats // 4), torch)
            row.setdefault("render", []).append(dict(blocks=K, ms=round(med, 4), min_ms=round(lo, 4)))

        def denoise():
            rt.denoise_device(w, h, d_sum.data_ptr(), d_sq.data_ptr(), 4, d_out[0].data_ptr(), d_dws.data_ptr(), params=dn, stream=stream)

        def tonemap():
            rt.tonemap_device(w, h, d_full.data_ptr(), 1, d_rgba8_ptr=d_rgba.data_ptr(), params=aces, stream=stream)

        d_bws = torch.zeros(rt.bloom_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        bp = rt.bloom_params(levels=5)

        def bloom():
            rt.bloom_device(w, h, d_full.data_ptr(), 1, d_out[0].data_ptr(), d_bws.data_ptr(), params=bp, stream=stream)

        for name, fn in (("denoise", denoise), ("tonemap", tonemap), ("bloom", bloom)):
            med, lo = timed(fn, args.repeats, torch)
            row[name + "_ms"], row[name + "_min_ms"] = round(med, 4), round(lo, 4)
        row["tonemap_gb_per_s"] = round(28 * w * h / row["tonemap_ms"] / 1e6, 1)   # 24 B read, 4 B written per pixel
        row["bloom_gb_per_s"] = round(bloom_least_bytes(w * h, 5, builtin_fused_max(w, h)) / row["bloom_ms"] / 1e6, 1)
        rows.append(row)
        del ds
    print(f"sources {source_hash()}; HIP events, 3 warm-up calls, median (minimum) of {args.repeats} calls; a synthetic stack of sums, spp = 4 per block, "
          "the default params (Gini, gain 1)")
    print("| frame | K | form (slots) | ms, means only | GB/s | ms, with M2 | GB/s |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        by = {(e["blocks"], e["form"], e["m2"]): e for e in r["robust"]}
        for K in FORMS:
            for form in (f for f in FORMS if f >= K):
                a, b = by[(K, form, False)], by[(K, form, True)]
                print(f"| {r['width']} x {r['height']} | {K} | {form}{' (built-in)' if form == K else ''} | {a['ms']:.4f} ({a['min_ms']:.4f}) | {a['gb_per_s']:.1f} | "
                      f"{b['ms']:.4f} ({b['min_ms']:.4f}) | {b['gb_per_s']:.1f} |")
    print("| frame | rt_denoise_device K = 4, ms | rt_tonemap_device ACES RGBA8, ms | its GB/s (28 B per pixel) | rt_bloom_device K = 5, ms | its GB/s | " +
          " | ".join(f"render of {K} x {max(1, 16 // K)} spp, ms" for K in FORMS) + " |")
    print("|---|---|---|---|---|---|" + "---|" * len(FORMS))
    for r in rows:
        print(f"| {r['width']} x {r['height']} | {r['denoise_ms']:.4f} ({r['denoise_min_ms']:.4f}) | {r['tonemap_ms']:.4f} ({r['tonemap_min_ms']:.4f}) | "
              f"{r['tonemap_gb_per_s']:.1f} | {r['bloom_ms']:.4f} ({r['bloom_min_ms']:.4f}) | {r['bloom_gb_per_s']:.1f} | " + " | ".join(f"{e['ms']:.3f} ({e['min_ms']:.3f})" for e in r["render"]) + " |")
    print(json.dumps(dict(tool="robust_speed", device=torch.cuda.get_device_name(0), repeats=args.repeats, sources=source_hash(), rows=rows)))


if __name__ == "__main__":
    main()
