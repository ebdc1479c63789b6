#!/usr/bin/env python3
"""MI355X.  What the film stage costs beside the tone-mapping stage, and what its smaller payloads save on the way to the host, on a
1200 x 800 frame of means:

    milliseconds per call (HIP events, after 3 warm-up calls; the median, the minimum and the spread max - min of --repeats calls) of
        rt_tonemap_device writing RGB8, and writing RGBA8      the existing stage, in the same session: the yardsticks
        rt_film_device writing RGBE, F32 and RGB16             clamp, exposure 1: the same reads, another encoder and store
    milliseconds per device-to-host copy into pinned memory (wall clock around the copy and its synchronisation, same warm-up and repeats) of
        the f64 frame (24 bytes per pixel)                     what a caller had to download for unclipped radiance before
        each payload above (3, 4, 4, 12 and 6 bytes per pixel)

    python tools/film_speed.py [--repeats 30]

The frame is a synthetic one of radiances 1e-3 .. 1e2 (the stage reads no scene).  Prints two tables (markdown, for DESIGN.md section 5
"Film output") and one JSON line; writes all of it to profiles/film_speed.txt."""
import argparse
import importlib
import json
import statistics
import sys
import time
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


def download(d_buf, repeats, torch):
    host = torch.empty(d_buf.shape, dtype=d_buf.dtype).pin_memory()
    for _ in range(3):
        host.copy_(d_buf)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        host.copy_(d_buf, non_blocking=True)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("rust-tracing_amd")
    stream = torch.cuda.current_stream().cuda_stream
    w, h = 1200, 800
    rng = np.random.default_rng(1)
    d_mean = torch.from_numpy(10.0 ** rng.uniform(-3.0, 2.0, size=(h, w, 3))).cuda()
    outs = {name: torch.zeros(n, dtype=torch.uint8, device="cuda")
            for name, n in (("rgb8", w * h * 3), ("rgba8", w * h * 4), ("rgbe", rt.film_bytes(w, h, "rgbe")), ("f32", rt.film_bytes(w, h, "f32")),
                            ("rgb16", rt.film_bytes(w, h, "rgb16")))}
    params = rt.tonemap_params()

    def tonemap(name):
        rt.tonemap_device(w, h, d_mean.data_ptr(), 1, **{f"d_{name}_ptr": outs[name].data_ptr()}, params=params, stream=stream)

    def film(name):
        rt.film_device(w, h, d_mean.data_ptr(), 1, name, outs[name].data_ptr(), params=params, stream=stream)

    calls = {}
    for name in ("rgb8", "rgba8"):
        calls[name] = timed(lambda: tonemap(name), args.repeats, torch)
    for name in ("rgbe", "f32", "rgb16"):
        calls[name] = timed(lambda: film(name), args.repeats, torch)
    copies = {"f64": download(d_mean, args.repeats, torch)}
    for name, buf in outs.items():
        copies[name] = download(buf, args.repeats, torch)
    bytes_pp = dict(f64=24, rgb8=3, rgba8=4, rgbe=4, f32=12, rgb16=6)
    label = dict(rgb8="rt_tonemap_device, RGB8", rgba8="rt_tonemap_device, RGBA8", rgbe="rt_film_device, RGBE", f32="rt_film_device, F32",
                 rgb16="rt_film_device, RGB16", f64="the f64 frame")
    lines = [f"film_speed: {w} x {h}, {torch.cuda.get_device_name(0)}, {args.repeats} repeats after 3 warm-up calls", "",
             "| call | output bytes per pixel | ms per call, median | minimum | spread (max - min) |", "|---|---|---|---|---|"]
    for name, s in calls.items():
        lines.append(f"| {label[name]} | {bytes_pp[name]} | {s['median_ms']:.4f} | {s['min_ms']:.4f} | {s['spread_ms']:.4f} |")
    lines += ["", "| download to pinned host memory | bytes per pixel | ms per copy, median | minimum | spread (max - min) |", "|---|---|---|---|---|"]
    for name, s in copies.items():
        lines.append(f"| {label[name] if name == 'f64' else name} | {bytes_pp[name]} | {s['median_ms']:.4f} | {s['min_ms']:.4f} | {s['spread_ms']:.4f} |")
    extra = calls["rgbe"]["median_ms"] - calls["rgba8"]["median_ms"]
    spread = max(calls["rgbe"]["spread_ms"], calls["rgba8"]["spread_ms"])
    lines += ["", f"RGBE call minus RGBA8 tone-map call: {extra:+.4f} ms (median); the larger run-to-run spread of the two: {spread:.4f} ms"]
    lines.append(json.dumps(dict(tool="film_speed", device=torch.cuda.get_device_name(0), repeats=args.repeats, width=w, height=h, calls=calls,
                                 downloads=copies)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out_dir = ROOT / "profiles"
    out_dir.mkdir(exist_ok=True)
    (out_dir / "film_speed.txt").write_text(text)


if __name__ == "__main__":
    main()
