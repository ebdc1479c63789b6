#!/usr/bin/env python3
"""MI355X.  What bloom costs beside the two scene-free stages it sits between: milliseconds per call (HIP events, after 3 warm-up
calls, the median and the minimum of --repeats calls) on a frame of means at 1200 x 800 and at 256 x 256, for

    rt_bloom_device, K = 1, 3, 5, 8       with the built-in choice of the levels' form
    rt_bloom_device, K = 5                with the one-launch LDS form forced up to stride 0 (never), 1 and 2: the A/B behind that choice
    rt_denoise_device, plain, K = 4       the filter in front of it, same frames, same session
    rt_tonemap_device, ACES, RGBA8        the stage behind it

    python tools/bloom_speed.py [--repeats 20]

The frame is a synthetic one of radiances 1e-3 .. 1e2 (the stage reads no scene).  Beside each bloom time stand the bytes the call's
launches must move at the least (the bright pass: 24 B read, 48 B written per pixel; a level in two passes: 24 + 24 B, then 24 + 24 B for
A and 48 B written; in one launch: 24 + 24 B read, 48 B written; the last level reads the frame again, 24 B, and writes the output alone)
and that figure over the median as GB/s.  Prints the tables (markdown, for DESIGN.md section 5 "Bloom") and one JSON line."""
import argparse
import importlib
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


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


def least_bytes(n_pixels, levels, fused_max):
    """bytes per call that the launches must read and write, from the shapes alone"""
    total = 24 + 48                                   # bright: the frame in, B0 and A out
    for k in range(levels):
        last = k == levels - 1
        fused = (1 << k) <= fused_max
        if not fused:
            total += 24 + 24                          # H pass
        total += 24 + 24                              # B (or H) and A in
        total += 24 + 24 if last else 48              # last: the frame in, the output; else B and A out
    return total * n_pixels


def builtin_fused_max(w, h):
    """the library's rule (rt_api.cpp): strides 1 and 2 as one launch on frames of at least 512 tiles of 64 x 16 pixels"""
    return 2 if -(-w // 64) * -(-h // 16) >= 512 else 0


def launches(levels, fused_max):
    return 1 + sum(1 if (1 << k) <= fused_max else 2 for k in range(levels))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("rust-tracing_amd")
    lib = rt.amd_lib()
    stream = torch.cuda.current_stream().cuda_stream
    lib.rt_debug_set_bloom_fused(-1)
    rows = []
    for w, h in ((1200, 800), (256, 256)):
        rng = np.random.default_rng(1)
        mean = 10.0 ** rng.uniform(-3.0, 2.0, size=(h, w, 3))
        d_mean = torch.from_numpy(mean).cuda()
        d_sq = torch.from_numpy(mean * mean * 1.5).cuda()          # sums of squares of 4 samples around the mean, for the denoiser
        d_sum = torch.from_numpy(mean * 4.0).cuda()
        d_sq4 = d_sq * 4.0
        d_out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
        d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        d_ws = torch.zeros(rt.bloom_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        d_dws = torch.zeros(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        aces, dn = rt.tonemap_params(op="aces"), rt.denoise_params(iterations=4)

        def bloom(params):
            rt.bloom_device(w, h, d_mean.data_ptr(), 1, d_out.data_ptr(), d_ws.data_ptr(), params=params, stream=stream)

        def denoise():
            rt.denoise_device(w, h, d_sum.data_ptr(), d_sq4.data_ptr(), 4, d_out.data_ptr(), d_dws.data_ptr(), params=dn, stream=stream)

        def tonemap():
            rt.tonemap_device(w, h, d_mean.data_ptr(), 1, d_rgba8_ptr=d_rgba.data_ptr(), params=aces, stream=stream)

        builtin = builtin_fused_max(w, h)
        row = dict(width=w, height=h, fused_builtin=builtin, bloom=[], ab=[])
        for levels in (1, 3, 5, 8):
            params = rt.bloom_params(levels=levels)
            med, lo = timed(lambda: bloom(params), args.repeats, torch)
            b = least_bytes(w * h, levels, builtin)
            row["bloom"].append(dict(levels=levels, ms=round(med, 4), min_ms=round(lo, 4), launches=launches(levels, builtin), bytes=b,
                                     gb_per_s=round(b / med / 1e6, 1)))
        params = rt.bloom_params(levels=5)
        reference = None
        for fused_max in (0, 1, 2):
            lib.rt_debug_set_bloom_fused(fused_max)
            med, lo = timed(lambda: bloom(params), args.repeats, torch)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            if reference is None:
                reference = got
            assert np.array_equal(got.view(np.uint64), reference.view(np.uint64)), "the forms must give the same bits"
            b = least_bytes(w * h, 5, fused_max)
            row["ab"].append(dict(fused_max=fused_max, ms=round(med, 4), min_ms=round(lo, 4), launches=launches(5, fused_max), bytes=b,
                                  gb_per_s=round(b / med / 1e6, 1)))
        lib.rt_debug_set_bloom_fused(-1)
        for name, fn in (("denoise", denoise), ("tonemap", tonemap)):
            med, lo = timed(fn, args.repeats, torch)
            row[name + "_ms"], row[name + "_min_ms"] = round(med, 4), round(lo, 4)
        rows.append(row)
    print("(the built-in rule unless stated: one launch per level up to stride " + ", ".join(f"{r['fused_builtin'] or 'never'} at {r['width']} x {r['height']}" for r in rows) +
          "; median of the calls, their minimum in brackets)")
    print("| frame | bloom K = 1, ms | K = 3 | K = 5 | K = 8 | rt_denoise_device K = 4, ms | rt_tonemap_device ACES RGBA8, ms |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['width']} x {r['height']} | " + " | ".join(f"{b['ms']:.4f} ({b['min_ms']:.4f})" for b in r["bloom"]) +
              f" | {r['denoise_ms']:.4f} ({r['denoise_min_ms']:.4f}) | {r['tonemap_ms']:.4f} ({r['tonemap_min_ms']:.4f}) |")
    print("| frame | K | launches | least bytes moved, MB | GB/s at the median |")
    print("|---|---|---|---|---|")
    for r in rows:
        for b in r["bloom"]:
            print(f"| {r['width']} x {r['height']} | {b['levels']} | {b['launches']} | {b['bytes'] / 1e6:.1f} | {b['gb_per_s']:.1f} |")
    print("| frame | K = 5, one launch up to stride | launches | ms | least bytes moved, MB | GB/s at the median |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        for b in r["ab"]:
            print(f"| {r['width']} x {r['height']} | {b['fused_max'] or 'never'} | {b['launches']} | {b['ms']:.4f} ({b['min_ms']:.4f}) | {b['bytes'] / 1e6:.1f} | {b['gb_per_s']:.1f} |")
    print(json.dumps(dict(tool="bloom_speed", device=torch.cuda.get_device_name(0), repeats=args.repeats, rows=rows)))


if __name__ == "__main__":
    main()
