#!/usr/bin/env python3
"""What rendering V views in one launch (rt_render_views_device) buys over V rt_render_device calls.  Not part of bench.py.

  For each workload and V in {1, 8, 64} orbit views (view k with seed 1 + k):
    (a) one rt_render_views_device call,
    (b) V rt_render_device calls back to back on the same stream, the existing path, one camera per call,
  each timed with HIP events around the enqueues and one final synchronisation: 1 warm-up and --reps timed repetitions, (a) and (b)
  alternating; Msamples/s from the median.  Both write the same bits (checked once per row).  V = 1 is the price of the mode itself.

  Workloads: C1 (random-spheres 400x225, 10 spp, depth 10: LDS spheres kernel), Cornell 128x128 at 16 spp (quads and frames kernel),
  final_scene 128x128 at 8 spp (scene gathered from global memory).

Usage: python tools/views_speed.py [--out FILE] [--views 1 8 64] [--reps 5]"""
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
    "c1 random-spheres 400x225x10spp d10": dict(scene=0, width=400, aspect=16.0 / 9.0, spp=10, depth=10),
    "cornell 128x128x16spp d50": dict(scene=6, width=128, aspect=1.0, spp=16, depth=50),
    "final_scene 128x128x8spp d40": dict(scene=8, width=128, aspect=1.0, spp=8, depth=40, earth_image="synthetic:1024x512"),
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


def measure(name, cfg, n_views, reps, log):
    hs = rt.HostScene(cfg["scene"], width=cfg["width"], aspect=cfg["aspect"], spp=cfg["spp"], depth=cfg["depth"],
                      earth_image=cfg.get("earth_image"))
    ds = rt.DeviceScene(hs)
    views = rt.orbit_views(hs, n_views, 1)
    frame = hs.width * hs.height * 3
    stream = torch.cuda.current_stream().cuda_stream
    d_a = torch.zeros(n_views * frame, dtype=torch.float64, device="cuda")
    d_b = torch.zeros(n_views * frame, dtype=torch.float64, device="cuda")
    cams = [rt.Camera.from_buffer_copy(bytes(views[k].camera)) for k in range(n_views)]
    params = [rt.render_params(seed=int(views[k].seed)) for k in range(n_views)]
    one = rt.render_params()

    def batched():
        ds.render_views_device(one, views, d_a.data_ptr(), stream)

    ptrs = [d_b[k * frame:].data_ptr() for k in range(n_views)]  # (outside the timed window: (b) is the calls alone)

    def looped():
        for k in range(n_views):
            ds.render_device(params[k], ptrs[k], stream, camera=cams[k])

    batched(); looped()  # warm-up: scratch, code objects
    torch.cuda.synchronize()
    same = bool(torch.equal(d_a.view(torch.int64), d_b.view(torch.int64)))
    ta, tb = [], []
    for _ in range(reps):  # alternating
        ta.append(event_ms(batched))
        tb.append(event_ms(looped))
    samples = n_views * hs.width * hs.height * cfg["spp"] / 1e6
    ma, mb = statistics.median(ta), statistics.median(tb)
    log(f"{name:38s} {n_views:3d}  {samples / (ma / 1e3):9.1f} {samples / (mb / 1e3):9.1f}  {mb / ma:6.3f}   {ma:8.3f} {mb:8.3f}   "
        f"{min(ta):.3f}-{max(ta):.3f} / {min(tb):.3f}-{max(tb):.3f}   {'yes' if same else 'NO'}")
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"tools/views_speed.py: (a) one rt_render_views_device call against (b) V rt_render_device calls on one stream; {torch.cuda.get_device_name(0)}")
    log(f"sources {source_hash()}; HIP events, 1 warm-up + {args.reps} timed repetitions alternating, medians; Msamples/s")
    log(f"{'workload':38s}   V   (a) views  (b) loop   (a)/(b)   ms (a)   ms (b)    range ms (a) / (b)            same bits")
    ok = True
    for name, cfg in WORKLOADS.items():
        for v in args.views:
            ok = measure(name, cfg, v, args.reps, log) and ok
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
