#!/usr/bin/env python3
"""MI355X.  What the tone-mapping stage costs beside the output stage it stands in for: milliseconds per call (HIP events, after 3
warm-up calls, the median and the minimum of --repeats calls) on a frame of means at 1200 x 800 and at 256 x 256, RGBA8 output, for

    rt_resolve_rgba8_device                          the existing stage, in the same session: the yardstick
    rt_tonemap_device, clamp                         the same reads and writes, the stage's code
    rt_tonemap_device, ACES                          the curve's two divisions and six multiply-adds more per value
    rt_tonemap_device, ACES + auto-exposure          the reduction's levels in front of it
    rt_log_average_luminance_device                  the reduction alone

    python tools/tonemap_speed.py [--repeats 20]

The frame is a synthetic one of radiances 1e-3 .. 1e2 (the stage reads no scene).  Prints one table (markdown, for DESIGN.md section 5
"Tone mapping") and one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("rust-tracing_amd")
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for w, h in ((1200, 800), (256, 256)):
        rng = np.random.default_rng(1)
        d_mean = torch.from_numpy(10.0 ** rng.uniform(-3.0, 2.0, size=(h, w, 3))).cuda()
        d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        d_out4 = torch.zeros(4, dtype=torch.float64, device="cuda")
        d_ws = torch.zeros(rt.tonemap_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        clamp, aces, auto = rt.tonemap_params(), rt.tonemap_params(op="aces"), rt.tonemap_params(op="aces", auto_key=0.18)

        def resolve():
            rt.resolve_rgba8_device(w, h, d_mean.data_ptr(), d_rgba.data_ptr(), stream)

        def tonemap(params):
            rt.tonemap_device(w, h, d_mean.data_ptr(), 1, d_rgba8_ptr=d_rgba.data_ptr(), d_workspace_ptr=d_ws.data_ptr(), params=params, stream=stream)

        def log_average():
            rt.log_average_luminance_device(w, h, d_mean.data_ptr(), 1, d_out4.data_ptr(), d_ws.data_ptr(), stream=stream)

        row = dict(width=w, height=h)
        for name, fn in (("resolve", resolve), ("clamp", lambda: tonemap(clamp)), ("aces", lambda: tonemap(aces)), ("aces_auto", lambda: tonemap(auto)),
                         ("log_average", log_average)):
            med, lo = timed(fn, args.repeats, torch)
            row[name + "_ms"], row[name + "_min_ms"] = round(med, 4), round(lo, 4)
        rows.append(row)
    print("| frame | rt_resolve_rgba8_device, ms | tonemap clamp, ms | tonemap ACES, ms | ACES + auto-exposure, ms | log-average alone, ms |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['width']} x {r['height']} | " + " | ".join(f"{r[k + '_ms']:.4f} ({r[k + '_min_ms']:.4f})" for k in ("resolve", "clamp", "aces", "aces_auto", "log_average")) + " |")
    print("(median of the calls, their minimum in brackets)")
    print(json.dumps(dict(tool="tonemap_speed", device=torch.cuda.get_device_name(0), repeats=args.repeats, rows=rows)))


if __name__ == "__main__":
    main()
