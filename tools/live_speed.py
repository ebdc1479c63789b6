#!/usr/bin/env python3
"""Displayed frames per second of live refinement (rt_render_mean_device with the fused RGBA8 frame).  Not part of bench.py.

  A displayed frame is one pass of K samples per pixel followed by the bytes to show.  For each frame size and K in {1, 8}, --frames
  passes in a row, pass f over the samples [f K, (f + 1) K), continuing one buffer:
    (a) rt_render_mean_device(d_mean, d_rgba8): the render launches and ONE reduction that folds the samples into the running mean
        and writes the RGBA8 frame,
    (b) what a caller had before: rt_render_device(accumulate) onto the sums, then rt_resolve_rgb8_device at spp = (f + 1) K
        (RGB8: the repacking to RGBA on the host that such a caller needs is not timed, which flatters (b)),
  each timed with HIP events around the enqueues and one final synchronisation: 1 warm-up and --reps timed repetitions, (a) and (b)
  alternating; frames per second from the median.  First the two routes must trace the same samples: over [0, 1) the mean is
  0 + (c - 0) / 1 = c and the sum is 0 + c, so the two buffers must hold the same bits.

  Frames: C1's (random-spheres 400x225, depth 10) and C2's (random-spheres 1200x800, depth 50).

Usage: python tools/live_speed.py [--out FILE] [--passes 1 8] [--frames 8] [--reps 5]"""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402
from source_hash import source_hash  # noqa: E402

rt = importlib.import_module("rust-tracing_amd")
WORKLOADS = {
    "c1 random-spheres 400x225 d10": dict(scene=0, width=400, aspect=16.0 / 9.0, depth=10),
    "c2 random-spheres 1200x800 d50": dict(scene=0, width=1200, aspect=1.5, depth=50),
}


def event_ms(fn):
    """milliseconds between two events around fn's enqueues, after one final synchronisation"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def measure(name, cfg, k, frames, reps, log):
    hs = rt.HostScene(cfg["scene"], width=cfg["width"], aspect=cfg["aspect"], spp=k * frames, depth=cfg["depth"])
    ds = rt.DeviceScene(hs)
    w, h = hs.width, hs.height
    stream = torch.cuda.current_stream().cuda_stream
    d_mean = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    d_sum = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    d_rgba8 = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    d_rgb8 = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")

    # the same samples: [0, 1) through either route leaves the sample's colour
    ds.render_mean_device(rt.render_params(seed=1, sample_begin=0, sample_end=1), d_mean.data_ptr(), d_rgba8.data_ptr(), stream)
    ds.render_device(rt.render_params(seed=1, sample_begin=0, sample_end=1), d_sum.data_ptr(), stream)
    torch.cuda.synchronize()
    same = bool(torch.equal(d_mean.view(torch.int64), d_sum.view(torch.int64)))

    mean_params = [rt.render_params(seed=1, sample_begin=f * k, sample_end=(f + 1) * k) for f in range(frames)]
    sum_params = [rt.render_params(seed=1, sample_begin=f * k, sample_end=(f + 1) * k, accumulate=f > 0) for f in range(frames)]

    def live():
        for f in range(frames):
            ds.render_mean_device(mean_params[f], d_mean.data_ptr(), d_rgba8.data_ptr(), stream)

    def summed():
        for f in range(frames):
            ds.render_device(sum_params[f], d_sum.data_ptr(), stream)
            rt.resolve_rgb8_device(w, h, (f + 1) * k, d_sum.data_ptr(), d_rgb8.data_ptr(), stream)

    live(); summed()  # warm-up: scratch, code objects
    torch.cuda.synchronize()
    # (the two frames need not be equal byte for byte — a running mean is not sum / n in its last bits — but nearly all bytes are)
    shown = d_rgba8.view(h * w, 4)[:, :3].reshape(-1)
    differing = int((shown != d_rgb8).sum().item())
    ta, tb = [], []
    for _ in range(reps):  # alternating
        ta.append(event_ms(live))
        tb.append(event_ms(summed))
    ma, mb = statistics.median(ta), statistics.median(tb)
    log(f"{name:32s} {k:3d}  {frames / (ma / 1e3):9.1f} {frames / (mb / 1e3):9.1f}  {mb / ma:6.3f}   {ma:8.3f} {mb:8.3f}   "
        f"{min(ta):.3f}-{max(ta):.3f} / {min(tb):.3f}-{max(tb):.3f}   {'yes' if same else 'NO':>4s}   {differing} of {w * h * 3}")
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

    log(f"tools/live_speed.py: (a) rt_render_mean_device with the fused RGBA8 frame against (b) rt_render_device(accumulate) + "
        f"rt_resolve_rgb8_device; {torch.cuda.get_device_name(0)}")
    log(f"sources {source_hash()}; {args.frames} displayed frames in a row, K samples per pixel each; HIP events, 1 warm-up + {args.reps} "
        f"timed repetitions alternating, medians; frames per second")
    log(f"{'frame':32s}   K   (a) live   (b) sum   (a)/(b)   ms (a)   ms (b)    range ms (a) / (b)            same samples   bytes that differ, last frame")
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
