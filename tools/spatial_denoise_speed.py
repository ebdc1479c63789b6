#!/usr/bin/env python3
"""What the FIRST displayed frame of the live route costs with the spatial variance estimate.  Not part of bench.py; live_speed.py's method.

  The first displayed frame is one pass over sample 0 followed by the bytes to show.  For each frame size, timed from sample_begin = 0:
    (a) the plain live route: rt_render_mean_device(d_mean, d_rgba8),
    (b) --live-denoise as it is: rt_render_mean_moments_device(d_mean, d_m2), then rt_denoise_mean_device at samples = 1 — launched in
        full, and its output is its input,
    (c) the spatial route: (b)'s reduction, then rt_denoise_mean_spatial_device at samples = 1 (defaults: R = 1),
  and, alongside, the filter alone on the frames (b) left: rt_denoise_mean_spatial_device at samples = 1 for R = 1, 2, 3 and the guided
  form at R = 1 (the spatial prepare and K = 4 iterations), against rt_denoise_mean_device at samples = 2 (the M2 prepare and the same
  iterations).  Each is timed with HIP events around the enqueues and one final synchronisation: 1 warm-up and --reps timed
  repetitions, alternating; medians and ranges.

  Frames: the bench scene (random spheres) at 400x225 (depth 10) and at 1200x800 (depth 50).

Usage: python tools/spatial_denoise_speed.py [--out FILE] [--reps 5]"""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402
from live_speed import WORKLOADS, event_ms  # noqa: E402
from source_hash import source_hash  # noqa: E402

rt = importlib.import_module("rust-tracing_amd")


def measure(name, cfg, reps, log):
    hs = rt.HostScene(cfg["scene"], width=cfg["width"], aspect=cfg["aspect"], spp=2, depth=cfg["depth"])
    ds, ds_albedo = rt.DeviceScene(hs), rt.DeviceScene(hs, albedo=True)
    w, h = hs.width, hs.height
    stream = torch.cuda.current_stream().cuda_stream

    def frame():
        return torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")

    d_plain, d_mean, d_m2, d_alb, d_shown = frame(), frame(), frame(), frame(), frame()
    d_rgba8 = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    d_ws = torch.empty(rt.denoise_albedo_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    first = rt.render_params(seed=1, sample_begin=0, sample_end=1)
    ds_albedo.render_mean_device(first, d_alb.data_ptr(), 0, stream, camera=rt.albedo_camera(hs.camera))
    out = dict(d_rgba8_ptr=d_rgba8.data_ptr(), stream=stream)

    def plain():
        ds.render_mean_device(first, d_plain.data_ptr(), d_rgba8.data_ptr(), stream)

    def today():
        ds.render_mean_moments_device(first, d_mean.data_ptr(), d_m2.data_ptr(), 0, stream)
        rt.denoise_mean_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), 1, d_shown.data_ptr(), d_ws.data_ptr(), **out)

    def spatial():
        ds.render_mean_moments_device(first, d_mean.data_ptr(), d_m2.data_ptr(), 0, stream)
        rt.denoise_mean_spatial_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), 1, d_shown.data_ptr(), d_ws.data_ptr(), **out)

    def filter_spatial(radius):
        sp = rt.denoise_spatial_params(window_radius=radius)
        return lambda: rt.denoise_mean_spatial_device(w, h, d_mean.data_ptr(), 0, 1, d_shown.data_ptr(), d_ws.data_ptr(), spatial=sp, **out)

    def filter_guided():
        rt.denoise_albedo_mean_spatial_device(w, h, d_mean.data_ptr(), 0, 1, d_alb.data_ptr(), d_shown.data_ptr(), d_ws.data_ptr(), **out)

    def filter_m2():
        rt.denoise_mean_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), 2, d_shown.data_ptr(), d_ws.data_ptr(), **out)

    routes = [("(a) plain", plain), ("(b) today", today), ("(c) spatial", spatial), ("filter spatial R=1", filter_spatial(1)),
              ("filter spatial R=2", filter_spatial(2)), ("filter spatial R=3", filter_spatial(3)), ("filter guided spatial R=1", filter_guided),
              ("filter M2 (samples 2)", filter_m2)]
    for _, fn in routes:  # warm-up: scratch, code objects
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(d_plain.view(torch.int64), d_mean.view(torch.int64)))
    times = {label: [] for label, _ in routes}
    for _ in range(reps):  # alternating
        for label, fn in routes:
            times[label].append(event_ms(fn))
    for label, _ in routes:
        t = times[label]
        log(f"{name:32s} {label:28s} {statistics.median(t):9.4f} ms   {min(t):.4f}-{max(t):.4f}   {'yes' if same else 'NO':>4s}")
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"tools/spatial_denoise_speed.py: the first displayed frame (sample 0) through (a) rt_render_mean_device, (b) rt_render_mean_moments_device + "
        f"rt_denoise_mean_device and (c) + rt_denoise_mean_spatial_device; the filters alone; {torch.cuda.get_device_name(0)}")
    log(f"sources {source_hash()}; default filter parameters (K = 4); HIP events, 1 warm-up + {args.reps} timed repetitions alternating, medians")
    log(f"{'frame':32s} {'route':28s} {'median':>12s}   range ms      same mean")
    ok = True
    for name, cfg in WORKLOADS.items():
        ok = measure(name, cfg, args.reps, log) and ok
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
