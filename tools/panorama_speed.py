#!/usr/bin/env python3
"""MI355X.  What the cube-to-equirectangular resampler costs beside the stages around it, at 2048 x 1024 from F = 514, g = 1 faces:

    milliseconds per call (HIP events, after 3 warm-up calls; the median, the minimum and the spread max - min of --repeats calls) of
        rt_panorama_device                                     its output is compared bit for bit against the host mirror
        rt_tonemap_device writing RGBA8 on the same frame      the stage behind it, in the same session: the yardstick
        rt_render_views_device, the six faces at 16 spp        the stage in front of it (the Cornell box from inside; --render-repeats)

    python tools/panorama_speed.py [--repeats 30] [--render-repeats 3]

The resampler's faces are synthetic (the stage reads no scene).  Prints a table (markdown, for DESIGN.md section 5 "Panorama") and one
JSON line; writes all of it to profiles/panorama_speed.txt."""
import argparse
import importlib
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), spread_ms=round(max(ms) - min(ms), 4))


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
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--render-repeats", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("rust-tracing_amd")
    stream = torch.cuda.current_stream().cuda_stream
    w, h, F, g, spp = 2048, 1024, 514, 1, 16
    rng = np.random.default_rng(1)
    faces = 10.0 ** rng.uniform(-3.0, 2.0, size=(6, F, F, 3))
    tables = rt.panorama_tables(w, h)
    d_faces, d_tables = torch.from_numpy(faces).cuda(), torch.from_numpy(tables).cuda()
    d_out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")

    def resample():
        rt.panorama_device(w, h, d_tables.data_ptr(), d_faces.data_ptr(), F, g, 1, d_out.data_ptr(), stream=stream)

    want = rt.panorama_host(w, h, faces, g, 1, tables=tables)
    calls = {"panorama": timed(resample, args.repeats, torch)}
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want.view(np.uint64)), "the device must give the mirror's bits"
    params = rt.tonemap_params()
    calls["tonemap_rgba8"] = timed(lambda: rt.tonemap_device(w, h, d_out.data_ptr(), 1, d_rgba8_ptr=d_rgba.data_ptr(), params=params, stream=stream),
                                   args.repeats, torch)
    hs = rt.HostScene(6, scene_seed=1, width=64, aspect=1.0, spp=spp, depth=50)   # cornell_box
    ds = rt.DeviceScene(hs, device=0)
    views = ds.panorama_views(F, g, (278.0, 278.0, 278.0), 1)
    d_stack = torch.zeros((6, F, F, 3), dtype=torch.float64, device="cuda")
    rp = rt.render_params(sample_end=spp)
    calls["render_six_faces_16spp"] = timed(lambda: ds.render_views_device(rp, views, d_stack.data_ptr(), stream), args.render_repeats, torch)
    moved = (6 * F * F + w * h) * 24   # every texel read once, every output value written once
    label = {"panorama": "rt_panorama_device", "tonemap_rgba8": "rt_tonemap_device, RGBA8, the same frame",
                  "render_six_faces_16spp": f"rt_render_views_device, six {F} x {F} faces of the Cornell box, {spp} spp"}
    lines = [f"panorama_speed: {w} x {h} from F = {F}, g = {g}, {torch.cuda.get_device_name(0)}, {args.repeats} repeats after 3 warm-up calls "
             f"({args.render_repeats} for the render)", "", "| call | ms per call, median | minimum | spread (max - min) | GB/s of the least traffic |", "|---|---|---|---|---|"]
    for name, s in calls.items():
        rate = f"{moved / s['median_ms'] / 1e6:.0f}" if name.startswith("panorama") else ""
        lines.append(f"| {label[name]} | {s['median_ms']:.4f} | {s['min_ms']:.4f} | {s['spread_ms']:.4f} | {rate} |")
    lines.append("")
    lines.append(json.dumps(dict(tool="panorama_speed", device=torch.cuda.get_device_name(0), repeats=args.repeats, width=w, height=h, face_size=F,
                                 guard=g, calls=calls)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out_dir = ROOT / "profiles"
    out_dir.mkdir(exist_ok=True)
    (out_dir / "panorama_speed.txt").write_text(text)


if __name__ == "__main__":
    main()
