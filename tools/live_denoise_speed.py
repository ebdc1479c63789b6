#!/usr/bin/env python3
"""Displayed frames per second of the DENOISING live route against the plain live route.  Not part of bench.py; live_speed.py's method.

  A displayed frame is one pass of K samples per pixel followed by the bytes to show.  For each frame size and K in {1, 8}, --frames
  passes in a row, pass f over the samples [f K, (f + 1) K), continuing the running frames:
    (a) the plain live route: rt_render_mean_device(d_mean, d_rgba8),
    (b) the denoising route: rt_render_mean_moments_device(d_mean, d_m2), then rt_denoise_mean_device over (d_mean, d_m2, (f + 1) K)
        into a separate frame and its RGBA8 bytes,
    (c) the guided one: (b)'s reduction, rt_render_mean_device of the albedo scene over the same samples under the white-background
        camera, then rt_denoise_albedo_mean_device,
  each timed with HIP events around the enqueues and one final synchronisation: 1 warm-up and --reps timed repetitions, (a), (b) and
  (c) alternating; frames per second from the median.  First (a) and (b) must hold the same running mean, bit for bit.

  Frames: the bench scene (random spheres) at 400x225 (depth 10) and at 1200x800 (depth 50).

Usage: python tools/live_denoise_speed.py [--out FILE] [--passes 1 8] [--frames 8] [--reps 5]"""
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


def measure(name, cfg, k, frames, reps, log):
    hs = rt.HostScene(cfg["scene"], width=cfg["width"], aspect=cfg["aspect"], spp=k * frames, depth=cfg["depth"])
    ds, ds_albedo = rt.DeviceScene(hs), rt.DeviceScene(hs, albedo=True)
    white = rt.albedo_camera(hs.camera)
    w, h = hs.width, hs.height
    stream = torch.cuda.current_stream().cuda_stream

    def frame():
        return torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")

    d_plain, d_mean, d_m2, d_alb, d_shown = frame(), frame(), frame(), frame(), frame()
    d_rgba8 = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    d_ws = torch.empty(rt.denoise_albedo_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")  # (the plain filter uses two thirds)
    params = [rt.render_params(seed=1, sample_begin=f * k, sample_end=(f + 1) * k) for f in range(frames)]

    def plain():
        for f in range(frames):
            ds.render_mean_device(params[f], d_plain.data_ptr(), d_rgba8.data_ptr(), stream)

    def denoised():
        for f in range(frames):
            ds.render_mean_moments_device(params[f], d_mean.data_ptr(), d_m2.data_ptr(), 0, stream)
            rt.denoise_mean_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), (f + 1) * k, d_shown.data_ptr(), d_ws.data_ptr(),
                                   d_rgba8_ptr=d_rgba8.data_ptr(), stream=stream)

    def guided():
        for f in range(frames):
            ds.render_mean_moments_device(params[f], d_mean.data_ptr(), d_m2.data_ptr(), 0, stream)
            ds_albedo.render_mean_device(params[f], d_alb.data_ptr(), 0, stream, camera=white)
            rt.denoise_albedo_mean_device(w, h, d_mean.data_ptr(), d_m2.data_ptr(), (f + 1) * k, d_alb.data_ptr(), d_shown.data_ptr(),
                                          d_ws.data_ptr(), d_rgba8_ptr=d_rgba8.data_ptr(), stream=stream)

    plain(); denoised(); guided()  # warm-up: scratch, code objects
    torch.cuda.synchronize()
    same = bool(torch.equal(d_plain.view(torch.int64), d_mean.view(torch.int64)))
    ta, tb, tc = [], [], []
    for _ in range(reps):  # alternating
        ta.append(event_ms(plain))
        tb.append(event_ms(denoised))
        tc.append(event_ms(guided))
    ma, mb, mc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    log(f"{name:32s} {k:3d}  {frames / (ma / 1e3):9.1f} {frames / (mb / 1e3):9.1f} {frames / (mc / 1e3):9.1f}   {mb / ma:6.3f} {mc / ma:6.3f}   "
        f"{ma / frames:7.3f} {mb / frames:7.3f} {mc / frames:7.3f}   {min(ta):.3f}-{max(ta):.3f} / {min(tb):.3f}-{max(tb):.3f} / {min(tc):.3f}-{max(tc):.3f}   "
        f"{'yes' if same else 'NO':>4s}")
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"tools/live_denoise_speed.py: (a) rt_render_mean_device against (b) rt_render_mean_moments_device + rt_denoise_mean_device and "
        f"(c) with the albedo pass and rt_denoise_albedo_mean_device; {torch.cuda.get_device_name(0)}")
    log(f"sources {source_hash()}; {args.frames} displayed frames in a row, K samples per pixel each, default filter parameters; HIP events, "
        f"1 warm-up + {args.reps} timed repetitions alternating, medians")
    log(f"{'frame':32s}   K   fps (a)   fps (b)   fps (c)   (b)/(a) (c)/(a)  ms per frame (a) (b) (c)   range ms of {args.frames} frames (a) / (b) / (c)"
        f"                    same mean")
    ok = True
    for name, cfg in WORKLOADS.items():
        for k in args.passes:
            ok = measure(name, cfg, k, args.frames, args.reps, log) and ok
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
