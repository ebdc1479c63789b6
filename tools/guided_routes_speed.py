#!/usr/bin/env python3
"""What the edge guide costs on the means, spatial-variance and views routes of the denoiser.  Not part of bench.py.

  Per frame size, milliseconds per call — the median of three runs of 20 calls, each run timed with HIP events around its enqueues
  after one warm-up call, with the three runs' range — of
    the three new forms (rt_denoise_guided_mean_device at samples = 2, rt_denoise_guided_mean_spatial_device at samples = 1 with
    R = 1, rt_denoise_guided_views_device over 4 views), each with and without the albedo frame;
    the spatial prepare, at R = 1 and R = 3, with edges and without, as the spatial call at K = 1: the prepare and one stride-1
    iteration (the entry points launch no prepare on its own), so read the rows against each other and against the full calls;
    beside them the existing plain and albedo means, spatial and views calls, which a library without the new forms (--existing-only:
    the parent commit's build) measures as well.
  Inputs are synthetic frames (noisy gradients, a blocky palette guide): the filters' cost does not depend on the scene.

Usage: python tools/guided_routes_speed.py [--out FILE] [--existing-only] [--package DIR]"""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SIZES = ((1200, 800), (256, 256))
RUNS, CALLS, VIEWS = 3, 20, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--existing-only", action="store_true", help="only the calls that exist without the edge guide's new forms")
    ap.add_argument("--package", default=str(ROOT), help="the directory that holds the rust-tracing_amd package to measure")
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    import torch
    rt = importlib.import_module("rust-tracing_amd")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def ms_per_call(fn):
        fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(RUNS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            torch.cuda.synchronize()
            runs.append(a.elapsed_time(b) / CALLS)
        return statistics.median(runs), min(runs), max(runs)

    log(f"tools/guided_routes_speed.py: ms per call, median of {RUNS} runs of {CALLS} (range); default filter parameters unless stated; "
        f"{torch.cuda.get_device_name(0)}; package {'(this tree)' if args.package == str(ROOT) else 'given with --package'}"
        f"{', existing calls only' if args.existing_only else ''}")
    log(f"{'frame':10s} {'call':58s} {'median':>9s}   range")
    for w, h in SIZES:
        g = torch.Generator(device="cuda").manual_seed(w)
        n = w * h * 3
        stream = torch.cuda.current_stream().cuda_stream

        def noisy(k=1):
            return (0.2 + torch.rand(k * n, dtype=torch.float64, device="cuda", generator=g)).contiguous()

        yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
        ids = ((xx // 37) + 3 * (yy // 29)) % 26 + 1
        guide = torch.stack([0.5 * (ids % 3), 0.5 * ((ids // 3) % 3), 0.5 * (ids // 9)], dim=2).to(torch.float64).reshape(-1).contiguous()
        mean, m2, alb, out = noisy(), noisy() * 0.1, noisy(), torch.zeros(n, dtype=torch.float64, device="cuda")
        S, Q, A, E = noisy(VIEWS) * 8.0, noisy(VIEWS) * 16.0, noisy(VIEWS) * 4.0, guide.repeat(VIEWS) * 4.0
        out_v = torch.zeros(VIEWS * n, dtype=torch.float64, device="cuda")
        rgba = torch.zeros(VIEWS * w * h * 4, dtype=torch.uint8, device="cuda")
        ws = torch.empty(rt.denoise_workspace_bytes(w, h) * 2 * VIEWS, dtype=torch.uint8, device="cuda")  # four regions per view
        P = [t.data_ptr() for t in (mean, m2, alb, guide, out, S, Q, A, E, out_v)]
        d_mean, d_m2, d_alb, d_ids, d_out, d_S, d_Q, d_A, d_E, d_out_v = P
        kw = dict(d_rgba8_ptr=rgba.data_ptr(), stream=stream)
        calls = [
            ("rt_denoise_mean_device", lambda: rt.denoise_mean_device(w, h, d_mean, d_m2, 2, d_out, ws.data_ptr(), **kw)),
            ("rt_denoise_albedo_mean_device", lambda: rt.denoise_albedo_mean_device(w, h, d_mean, d_m2, 2, d_alb, d_out, ws.data_ptr(), **kw)),
            ("rt_denoise_mean_spatial_device R=1", lambda: rt.denoise_mean_spatial_device(w, h, d_mean, 0, 1, d_out, ws.data_ptr(), **kw)),
            ("rt_denoise_albedo_mean_spatial_device R=1",
             lambda: rt.denoise_albedo_mean_spatial_device(w, h, d_mean, 0, 1, d_alb, d_out, ws.data_ptr(), **kw)),
            (f"rt_denoise_views_device x{VIEWS}", lambda: rt.denoise_views_device(w, h, VIEWS, d_S, d_Q, 8, d_out_v, ws.data_ptr(), **kw)),
            (f"rt_denoise_albedo_views_device x{VIEWS}",
             lambda: rt.denoise_albedo_views_device(w, h, VIEWS, d_S, d_Q, 8, d_A, 4, d_out_v, ws.data_ptr(), **kw)),
        ]
        for R in (1, 3):
            sp = rt.denoise_spatial_params(window_radius=R)
            one = rt.denoise_params(iterations=1)
            calls.append((f"spatial prepare + 1 iteration, R={R}, plain",
                          lambda sp=sp, one=one: rt.denoise_mean_spatial_device(w, h, d_mean, 0, 1, d_out, ws.data_ptr(), spatial=sp, params=one, **kw)))
        if not args.existing_only:
            calls += [
                ("rt_denoise_guided_mean_device", lambda: rt.denoise_guided_mean_device(w, h, d_mean, d_m2, 2, 0, d_ids, d_out, ws.data_ptr(), **kw)),
                ("rt_denoise_guided_mean_device + albedo",
                 lambda: rt.denoise_guided_mean_device(w, h, d_mean, d_m2, 2, d_alb, d_ids, d_out, ws.data_ptr(), **kw)),
                ("rt_denoise_guided_mean_spatial_device R=1",
                 lambda: rt.denoise_guided_mean_spatial_device(w, h, d_mean, 0, 1, 0, d_ids, d_out, ws.data_ptr(), **kw)),
                ("rt_denoise_guided_mean_spatial_device R=1 + albedo",
                 lambda: rt.denoise_guided_mean_spatial_device(w, h, d_mean, 0, 1, d_alb, d_ids, d_out, ws.data_ptr(), **kw)),
                (f"rt_denoise_guided_views_device x{VIEWS}",
                 lambda: rt.denoise_guided_views_device(w, h, VIEWS, d_S, d_Q, 8, 0, 0, d_E, 4, d_out_v, ws.data_ptr(), **kw)),
                (f"rt_denoise_guided_views_device x{VIEWS} + albedo",
                 lambda: rt.denoise_guided_views_device(w, h, VIEWS, d_S, d_Q, 8, d_A, 4, d_E, 4, d_out_v, ws.data_ptr(), **kw)),
            ]
            for R in (1, 3):
                sp = rt.denoise_spatial_params(window_radius=R)
                one = rt.denoise_guided_params(iterations=1)
                calls.append((f"spatial prepare + 1 iteration, R={R}, edges",
                              lambda sp=sp, one=one: rt.denoise_guided_mean_spatial_device(w, h, d_mean, 0, 1, 0, d_ids, d_out, ws.data_ptr(), spatial=sp,
                                                                                         params=one, **kw)))
        for label, fn in calls:
            med, lo, hi = ms_per_call(fn)
            log(f"{w}x{h:<5d} {label:58s} {med:9.4f}   {lo:.4f}-{hi:.4f}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
