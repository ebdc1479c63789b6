#!/usr/bin/env python3
"""MI355X.  What the frame metrics cost: milliseconds per call (HIP events, --repeats calls after 3 warm-up calls: the median, the
minimum and max - min) on a 1200 x 800 frame for

    rt_frame_error_device                            six 8-byte loads per pixel, a five-accumulator tree
    rt_frame_noise_device, sums and means form       six loads per pixel, a three-accumulator tree
    rt_log_average_luminance_device                  the one-accumulator tree of the same shape: the yardstick
    rt_tonemap_device, clamp, RGBA8                  an elementwise pass over the same frame

and what the stop costs the live route: passes per second of `rtrace -l` at 1 sample per pass on the bench scene (scene 0), alone and
with `--live-stop 0` (the moments route, the noise reduced after every pass, its four doubles in the frame's own download; a threshold
that never stops the loop).  Each variant runs --loops times; the spread between the runs is printed beside the medians.

    python tools/metrics_speed.py [--repeats 30] [--passes 2000] [--loops 3] [--width 400] [--out profiles/metrics_speed.txt]

The kernel frames are synthetic (the calls read no scene).  Prints the tables (markdown, for DESIGN.md section 5 "Frame metrics") and one
JSON line, and writes the same text to --out."""
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
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), spread_ms=round(max(ms) - min(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--passes", type=int, default=2000)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "metrics_speed.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("rust-tracing_amd")
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    w, h = 1200, 800
    rng = np.random.default_rng(1)
    mean = 10.0 ** rng.uniform(-3.0, 2.0, size=(h, w, 3))
    d_mean = torch.from_numpy(mean).cuda()
    d_ref = torch.from_numpy(mean * (1.0 + rng.normal(0.0, 0.1, size=mean.shape))).cuda()
    d_sum = torch.from_numpy(mean * 8.0).cuda()
    d_sq = torch.from_numpy((mean * mean) * 12.0).cuda()
    d_m2 = torch.from_numpy((mean * mean) * 4.0).cuda()
    d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(8, dtype=torch.float64, device="cuda")
    d_ws = torch.zeros(max(rt.metrics_workspace_bytes(w, h), rt.tonemap_workspace_bytes(w, h)), dtype=torch.uint8, device="cuda")
    clamp = rt.tonemap_params()
    calls = [
        ("rt_frame_error_device", lambda: rt.frame_error_device(w, h, d_mean.data_ptr(), 1, d_ref.data_ptr(), 1, d_out.data_ptr(), d_ws.data_ptr(), stream=stream)),
        ("rt_frame_noise_device, sums", lambda: rt.frame_noise_device(w, h, "sums", d_sum.data_ptr(), d_sq.data_ptr(), 8, d_out.data_ptr(), d_ws.data_ptr(), stream=stream)),
        ("rt_frame_noise_device, means", lambda: rt.frame_noise_device(w, h, "means", d_mean.data_ptr(), d_m2.data_ptr(), 8, d_out.data_ptr(), d_ws.data_ptr(), stream=stream)),
        ("rt_log_average_luminance_device", lambda: rt.log_average_luminance_device(w, h, d_mean.data_ptr(), 1, d_out.data_ptr(), d_ws.data_ptr(), stream=stream)),
        ("rt_tonemap_device, clamp, RGBA8", lambda: rt.tonemap_device(w, h, d_mean.data_ptr(), 1, d_rgba8_ptr=d_rgba.data_ptr(), params=clamp, stream=stream)),
    ]
    kernels = {name: timed(fn, args.repeats, torch) for name, fn in calls}
    lines += [f"{w} x {h}, ms per call: {args.repeats} calls after 3 warm-up calls (HIP events)", "",
              "| call | median, ms | minimum, ms | max - min, ms |", "|---|---|---|---|"]
    lines += [f"| {name} | {r['median_ms']:.4f} | {r['min_ms']:.4f} | {r['spread_ms']:.4f} |" for name, r in kernels.items()]

    # the live route itself, 1 sample per pass on the bench scene: `rtrace -l` alone and with --live-stop 0, a threshold no pass reaches,
    # so both run the same passes; the loop's own clock ("Live: N frames, ..., T s") leaves the scene build out
    import re
    import subprocess
    import tempfile
    exe = rt.LIB_DIR / "rtrace"

    def loop(extra):
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([str(exe), "-s", "0", "--width", str(args.width), "--aspect", "1.5", "--spp", str(args.passes + 1), "-l", "-o", tmp + "/out", *extra],
                               capture_output=True, text=True, check=True)
        m = re.search(r"Live: (\d+) frames, \d+ samples per pixel in the last, ([0-9.]+)s", r.stdout)
        return int(m.group(1)) / float(m.group(2))

    loop([])  # warm-up: the binary, the driver
    live = {name: [round(loop(extra), 2) for _ in range(args.loops)]
            for name, extra in (("rtrace -l", []), ("rtrace -l --live-stop 0", ["--live-stop", "0"]))}
    lw, lh = args.width, int(args.width / 1.5)
    lines += ["", f"live route, bench scene at {lw} x {lh}, 1 sample per pass, {args.passes} passes; passes per second over {args.loops} runs "
              "(the loop's own clock, 0.01 s steps)", "", "| run | median | every run | max - min |", "|---|---|---|---|"]
    lines += [f"| {name} | {statistics.median(v):.2f} | {', '.join(f'{x:.2f}' for x in v)} | {max(v) - min(v):.2f} |" for name, v in live.items()]
    lines += ["", "(one run on one device; the spread columns are the only error bars it has)"]
    record = dict(tool="metrics_speed", device=torch.cuda.get_device_name(0), repeats=args.repeats, kernels=kernels, live=live,
                  live_frame=[lw, lh], passes=args.passes)
    lines.append(json.dumps(record))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
