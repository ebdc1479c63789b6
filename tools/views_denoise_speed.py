#!/usr/bin/env python3
"""What the views route's moments and the batched filter buy a caller who wants V denoised views.  Not part of bench.py.

  The bench scene (random-spheres, depth 50) at 16 spp, K = 4, default filter parameters, display bytes written; V orbit views (view
  k with seed 1 + k) at two workloads: 6 views of 256 x 256 (a cube map's worth) and 24 views of 400 x 225 (a turntable).  Routes:
    (a) one rt_render_views_moments_device call and one rt_denoise_views_device call;
    (b) what a caller had before: V x (rt_render_moments_device + rt_denoise_device), back to back on the same stream;
    (c) rt_render_views_device alone: the unfiltered views, what (a) is paid on top of;
    and the two filters alone on (a)'s moments: one rt_denoise_views_device call against V rt_denoise_device calls.
  Each is timed with HIP events around the enqueues and one final synchronisation: 1 warm-up and --reps timed repetitions, the routes
  alternating; medians and ranges in ms.  (a) and (b) write the same bits (checked once per workload).

Usage: python tools/views_denoise_speed.py [--out FILE] [--reps 5]"""
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
from views_speed import event_ms  # noqa: E402

rt = importlib.import_module("rust-tracing_amd")
SPP, K = 16, 4
WORKLOADS = {
    "6 views of 256x256": dict(width=256, aspect=1.0, views=6),
    "24 views of 400x225": dict(width=400, aspect=16.0 / 9.0, views=24),
}


def measure(name, cfg, reps, log):
    hs = rt.HostScene(0, width=cfg["width"], aspect=cfg["aspect"], spp=SPP, depth=50)
    ds = rt.DeviceScene(hs)
    n, w, h = cfg["views"], hs.width, hs.height
    views = rt.orbit_views(hs, n, 1)
    frame = w * h * 3
    stream = torch.cuda.current_stream().cuda_stream
    new = lambda count, dtype=torch.float64: torch.zeros(count, dtype=dtype, device="cuda")  # noqa: E731
    a_s, a_q, a_out, a_rgba = new(n * frame), new(n * frame), new(n * frame), new(n * w * h * 4, torch.uint8)
    b_s, b_q, b_out, b_rgba = new(n * frame), new(n * frame), new(n * frame), new(n * w * h * 4, torch.uint8)
    c_s = new(n * frame)
    ws_views = new(rt.denoise_views_workspace_bytes(w, h, n), torch.uint8)
    ws_one = new(rt.denoise_workspace_bytes(w, h), torch.uint8)
    cams = [rt.Camera.from_buffer_copy(bytes(views[k].camera)) for k in range(n)]
    params = [rt.render_params(seed=int(views[k].seed)) for k in range(n)]
    one = rt.render_params()
    dp = rt.denoise_params(iterations=K)
    at = lambda t, k, stride: t[k * stride:].data_ptr()  # noqa: E731  (pointers are taken outside the timed windows)
    pb = [(at(b_s, k, frame), at(b_q, k, frame), at(b_out, k, frame), at(b_rgba, k, w * h * 4)) for k in range(n)]
    pa = [(at(a_s, k, frame), at(a_q, k, frame), at(b_out, k, frame), at(b_rgba, k, w * h * 4)) for k in range(n)]

    def filter_views():
        rt.denoise_views_device(w, h, n, a_s.data_ptr(), a_q.data_ptr(), SPP, a_out.data_ptr(), ws_views.data_ptr(), d_rgba8_ptr=a_rgba.data_ptr(),
                                params=dp, stream=stream)

    def filter_loop(ptrs=pa):
        for s, q, out, rgba in ptrs:
            rt.denoise_device(w, h, s, q, SPP, out, ws_one.data_ptr(), d_rgba8_ptr=rgba, params=dp, stream=stream)

    def route_a():
        ds.render_views_moments_device(one, views, a_s.data_ptr(), a_q.data_ptr(), stream)
        filter_views()

    def route_b():
        for k in range(n):
            ds.render_moments_device(params[k], pb[k][0], pb[k][1], stream, camera=cams[k])
            rt.denoise_device(w, h, pb[k][0], pb[k][1], SPP, pb[k][2], ws_one.data_ptr(), d_rgba8_ptr=pb[k][3], params=dp, stream=stream)

    def route_c():
        ds.render_views_device(one, views, c_s.data_ptr(), stream)

    routes = [("(a) views moments + views filter", route_a), ("(b) V x (moments + filter)", route_b), ("(c) views render alone", route_c),
              ("views filter alone", filter_views), ("V single-frame filters alone", filter_loop)]
    for _, fn in routes:  # warm-up: scratch, code objects, the pixel list of the frame size
        fn()
    torch.cuda.synchronize()
    route_a(); route_b()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y))
               for x, y in ((a_s, b_s), (a_q, b_q), (a_out, b_out), (a_rgba, b_rgba)))
    times = {label: [] for label, _ in routes}
    for _ in range(reps):  # alternating
        for label, fn in routes:
            times[label].append(event_ms(fn))
    log(f"{name}, {w}x{h}, {SPP} spp, K = {K}; (a) and (b) write the same bits: {'yes' if same else 'NO'}")
    med = {label: statistics.median(t) for label, t in times.items()}
    for label, t in times.items():
        log(f"    {label:36s} median {med[label]:8.3f} ms   range {min(t):.3f}-{max(t):.3f}")
    log(f"    (b)/(a) {med[routes[1][0]] / med[routes[0][0]]:.3f}   (a)/(c) {med[routes[0][0]] / med[routes[2][0]]:.3f}   "
        f"V single-frame filters / views filter {med[routes[4][0]] / med[routes[3][0]]:.3f}   "
        f"views filter per view {med[routes[3][0]] / n:.4f} ms, single-frame filter per call {med[routes[4][0]] / n:.4f} ms")
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

    log(f"tools/views_denoise_speed.py: denoised views through the views route against one call pair per view; {torch.cuda.get_device_name(0)}")
    log(f"sources {source_hash()}; the bench scene; HIP events, 1 warm-up + {args.reps} timed repetitions, the routes alternating")
    ok = True
    for name, cfg in WORKLOADS.items():
        ok = measure(name, cfg, args.reps, log) and ok
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
