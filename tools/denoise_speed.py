#!/usr/bin/env python3
"""MI355X.  What the denoiser costs beside the render it cleans up: milliseconds per rt_denoise_device call (HIP events, after a
warm-up, the median of --repeats calls) at K = 4 with the display bytes, for the bench scene at 1200 x 800 and at 256 x 256, and
beside each the milliseconds of the 16-spp rt_render_moments_device of the same frame, measured the same way.

    python tools/denoise_speed.py [--repeats 20] [--iterations 4] [--albedo | --edges]

Prints one table row per frame (markdown, for DESIGN.md section 5 "Denoise") and one JSON line.  --albedo: the albedo-guided filter's
table instead (DESIGN.md section 5 "Albedo-guided denoise") — beside the moments render the milliseconds of the albedo pass (the
albedo scene's rt_render_device over the same samples under the white-background camera), of rt_denoise_albedo_device and of the
plain rt_denoise_device, all measured the same way in the same run.  --edges: the edge-guided filter's table (DESIGN.md section 5
"Edge-guided denoise") — the albedo table's columns and beside them the milliseconds of the ID pass (the surface-ID scene's
rt_render_device over the same samples under the black-background camera) and of rt_denoise_guided_device in its two modes, the ID
frame alone and beside the albedo frame."""
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
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--albedo", action="store_true")
    ap.add_argument("--edges", action="store_true")
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("rust-tracing_amd")
    rows = []
    for width, aspect in ((1200, 1.5), (256, 1.0)):
        hs = rt.HostScene(0, width=width, aspect=aspect, spp=args.spp, depth=50)
        w, h = hs.width, hs.height
        ds = rt.DeviceScene(hs)
        stream = torch.cuda.current_stream().cuda_stream
        d_s = torch.zeros(3 * w * h, dtype=torch.float64, device="cuda")
        d_q, d_out = torch.zeros_like(d_s), torch.zeros_like(d_s)
        d_b = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
        d_ws = torch.empty(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        p = rt.render_params(seed=1, sample_end=args.spp)
        dp = rt.denoise_params(iterations=args.iterations)

        def render():
            ds.render_moments_device(p, d_s.data_ptr(), d_q.data_ptr(), stream)

        def denoise():
            rt.denoise_device(w, h, d_s.data_ptr(), d_q.data_ptr(), args.spp, d_out.data_ptr(), d_ws.data_ptr(), d_rgba8_ptr=d_b.data_ptr(),
                              params=dp, stream=stream)

        render_ms, render_min = timed(render, args.repeats, torch)
        denoise_ms, denoise_min = timed(denoise, args.repeats, torch)
        rows.append(dict(width=w, height=h, spp=args.spp, iterations=args.iterations, render_ms=round(render_ms, 4), render_min_ms=round(render_min, 4),
                         denoise_ms=round(denoise_ms, 4), denoise_min_ms=round(denoise_min, 4), share=round(denoise_ms / (render_ms + denoise_ms), 4)))
        if args.albedo or args.edges:
            da = rt.DeviceScene(hs, albedo=True)
            white = rt.albedo_camera(hs.camera)
            d_a = torch.zeros_like(d_s)
            d_ws2 = torch.empty(rt.denoise_albedo_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
            dap = rt.denoise_albedo_params(iterations=args.iterations)

            def albedo_pass():
                da.render_device(p, d_a.data_ptr(), stream, camera=white)

            def guided():
                rt.denoise_albedo_device(w, h, d_s.data_ptr(), d_q.data_ptr(), args.spp, d_a.data_ptr(), args.spp, d_out.data_ptr(), d_ws2.data_ptr(),
                                         d_rgba8_ptr=d_b.data_ptr(), params=dap, stream=stream)

            albedo_ms, albedo_min = timed(albedo_pass, args.repeats, torch)
            guided_ms, guided_min = timed(guided, args.repeats, torch)
            rows[-1].update(albedo_ms=round(albedo_ms, 4), albedo_min_ms=round(albedo_min, 4), guided_ms=round(guided_ms, 4),
                            guided_min_ms=round(guided_min, 4), albedo_over_render=round(albedo_ms / render_ms, 4))
        if args.edges:
            di = rt.DeviceScene(hs, surface_ids=True)
            black = rt.surface_id_camera(hs.camera)
            d_e = torch.zeros_like(d_s)
            d_ws3 = torch.empty(rt.denoise_guided_workspace_bytes(w, h, True), dtype=torch.uint8, device="cuda")
            dgp = rt.denoise_guided_params(iterations=args.iterations)

            def id_pass():
                di.render_device(p, d_e.data_ptr(), stream, camera=black)

            def edges(with_albedo):
                rt.denoise_guided_device(w, h, d_s.data_ptr(), d_q.data_ptr(), args.spp, d_a.data_ptr() if with_albedo else 0, args.spp, d_e.data_ptr(),
                                         args.spp, d_out.data_ptr(), d_ws3.data_ptr(), d_rgba8_ptr=d_b.data_ptr(), params=dgp, stream=stream)

            id_ms, id_min = timed(id_pass, args.repeats, torch)
            edges_ms, edges_min = timed(lambda: edges(False), args.repeats, torch)
            both_ms, both_min = timed(lambda: edges(True), args.repeats, torch)
            rows[-1].update(id_ms=round(id_ms, 4), id_min_ms=round(id_min, 4), edges_ms=round(edges_ms, 4), edges_min_ms=round(edges_min, 4),
                            both_ms=round(both_ms, 4), both_min_ms=round(both_min, 4), id_over_render=round(id_ms / render_ms, 4))
    if args.edges:
        print(f"| frame | {args.spp}-spp moments render, ms | albedo pass, ms | ID pass, ms | ID pass / moments render | plain filter K = {args.iterations}, ms | "
              "albedo-guided, ms | edges (ID frame), ms | albedo + edges, ms |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['width']} x {r['height']} | {r['render_ms']:.3f} | {r['albedo_ms']:.3f} | {r['id_ms']:.3f} | {100 * r['id_over_render']:.1f} % | "
                  f"{r['denoise_ms']:.3f} | {r['guided_ms']:.3f} | {r['edges_ms']:.3f} | {r['both_ms']:.3f} |")
        print(json.dumps(dict(tool="denoise_speed --edges", device=torch.cuda.get_device_name(0), repeats=args.repeats, rows=rows)))
        return
    if args.albedo:
        print(f"| frame | {args.spp}-spp moments render, ms | albedo pass, ms | albedo pass / moments render | guided filter K = {args.iterations}, ms | plain filter, ms |")
        print("|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['width']} x {r['height']} | {r['render_ms']:.3f} | {r['albedo_ms']:.3f} | {100 * r['albedo_over_render']:.1f} % | {r['guided_ms']:.3f} | {r['denoise_ms']:.3f} |")
        print(json.dumps(dict(tool="denoise_speed --albedo", device=torch.cuda.get_device_name(0), repeats=args.repeats, rows=rows)))
        return
    print(f"| frame | {args.spp}-spp moments render, ms | denoise K = {args.iterations}, ms | denoise share of the preview |")
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['width']} x {r['height']} | {r['render_ms']:.3f} | {r['denoise_ms']:.3f} | {100 * r['share']:.1f} % |")
    print(json.dumps(dict(tool="denoise_speed", device=torch.cuda.get_device_name(0), repeats=args.repeats, rows=rows)))


if __name__ == "__main__":
    main()
