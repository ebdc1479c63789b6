#!/usr/bin/env python3
"""MI355X.  What guided upsampling costs: milliseconds per rt_upsample_device call (HIP events, after 3 warm-up calls, the median and
the minimum of --repeats calls) for

    600 x 400 -> 1200 x 800 (F = 2),   300 x 200 -> 1200 x 800 (F = 4),   128 x 128 -> 256 x 256 (F = 2)

per kernel form (the direct one and the LDS one, forced through rt_debug_set_upsample_form; their results are compared bit for bit) and per
guide set (none, ID, albedo, both), beside rt_denoise_device (plain, K = 4) on the same full-size frame in the same session, and beside
the least bytes the call must move: the low frame in (24 B per low pixel), the records out and in again (32 B per low pixel and region,
twice), each guide in twice (24 B per full-size pixel for the prepare step and for the pixel's own value) and the output (24 B per
full-size pixel; no display bytes are asked for).

and, end to end, the displayed frames per second of `rtrace -l --live-denoise` on the flagship scene (random balls, 1200 x 800, depth
50) with and without `--upsample 2 --upsample-albedo --upsample-edges`: 256 displayed frames of K = 1 and of K = 8 samples per pixel,
from the time rtrace prints for its live loop — scene upload, the guide renders (once per session) and every frame's download included
— the two alternating, --live-reps runs each, the median and the range.

    python tools/upsample_speed.py [--repeats 20] [--live-reps 3]

The per-call frames are synthetic (the stage reads no scene).  Prints the tables (markdown, for DESIGN.md section 5 "Upsampling") and
one JSON line."""
import argparse
import importlib
import json
import re
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    sys.path.insert(0, p)

CASES = [(1200, 800, 2), (1200, 800, 4), (256, 256, 2)]
GUIDE_SETS = ("none", "edge", "albedo", "both")


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


def least_bytes(w, h, F, n_guides):
    low = -(-w // F) * -(-h // F)
    return low * (24 + 2 * 32 * (1 + n_guides)) + w * h * (24 + 2 * 24 * n_guides)


LIVE_FRAMES = 256
LIVE_FLAGS = ["--upsample", "2", "--upsample-albedo", "--upsample-edges"]


def live_fps(rt, k, upsampled):
    """displayed frames per second of one rtrace live session of LIVE_FRAMES passes of k samples per pixel"""
    with tempfile.TemporaryDirectory() as tmp:
        return _live_fps(rt, k, upsampled, str(Path(tmp) / "live"))


def _live_fps(rt, k, upsampled, out):
    spp = LIVE_FRAMES * k + 1     # the live loop settles on spp - 1 samples
    cmd = [str(rt.LIB_DIR / "rtrace"), "-s", "0", "--width", "1200", "--aspect", "1.5", "--spp", str(spp), "--depth", "50", "--seed", "1", "--scene-seed", "1",
           "-l", "--live-spp", str(k), "--live-denoise", *(LIVE_FLAGS if upsampled else []), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"rtrace failed ({r.returncode}): {r.stderr}")
    m = re.search(r"Live: (\d+) frames, (\d+) samples per pixel in the last, ([0-9.]+)s", r.stdout)
    assert m and int(m.group(1)) == LIVE_FRAMES and int(m.group(2)) == spp - 1, r.stdout
    return LIVE_FRAMES / float(m.group(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--live-reps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    import upsample_helpers as uh
    rt = importlib.import_module("rust-tracing_amd")
    lib = rt.amd_lib()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for w, h, F in CASES:
        low, spp, (A, n_a), (E, n_e) = uh.inputs(w, h, F, seed=1)
        d_low, d_alb, d_edge = (torch.from_numpy(a).cuda() for a in (low, A, E))
        d_out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
        d_ws = torch.zeros(rt.upsample_workspace_bytes(w, h, F), dtype=torch.uint8, device="cuda")
        params = rt.upsample_params(factor=F)
        mean = np.abs(np.random.default_rng(1).normal(size=(h, w, 3))) + 0.1
        d_sum, d_sq = torch.from_numpy(mean * 4.0).cuda(), torch.from_numpy(mean * mean * 6.0).cuda()
        d_dws = torch.zeros(rt.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
        dn = rt.denoise_params(iterations=4)

        def upsample(kind):
            rt.upsample_device(w, h, d_low.data_ptr(), spp, d_out.data_ptr(), d_ws.data_ptr(),
                               d_albedo_sum_ptr=d_alb.data_ptr() if kind in ("albedo", "both") else 0, albedo_spp=n_a,
                               d_edge_sum_ptr=d_edge.data_ptr() if kind in ("edge", "both") else 0, edge_spp=n_e, params=params, stream=stream)

        def denoise():
            rt.denoise_device(w, h, d_sum.data_ptr(), d_sq.data_ptr(), 4, d_out.data_ptr(), d_dws.data_ptr(), params=dn, stream=stream)

        row = dict(width=w, height=h, factor=F, tiles=-(-w // 32) * -(-h // 8), calls=[])
        row["denoise_ms"], row["denoise_min_ms"] = (round(v, 4) for v in timed(denoise, args.repeats, torch))
        for kind in GUIDE_SETS:
            reference = None
            for form in (0, 1):
                lib.rt_debug_set_upsample_form(form)
                med, lo = timed(lambda: upsample(kind), args.repeats, torch)
                torch.cuda.synchronize()
                got = d_out.cpu().numpy()
                if reference is None:
                    reference = got
                assert np.array_equal(got.view(np.uint64), reference.view(np.uint64)), "the forms must give the same bits"
                b = least_bytes(w, h, F, {"none": 0, "edge": 1, "albedo": 1, "both": 2}[kind])
                row["calls"].append(dict(guides=kind, form="lds" if form else "direct", ms=round(med, 4), min_ms=round(lo, 4), bytes=b,
                                         gb_per_s=round(b / med / 1e6, 1)))
        lib.rt_debug_set_upsample_form(-1)
        rows.append(row)
    print("(median of the calls, their minimum in brackets; rt_denoise_device is the plain filter, K = 4, on the full-size frame)")
    print("| low -> full | F | tiles | guides | direct form, ms | LDS form, ms | least bytes moved, MB | GB/s at the faster median | rt_denoise_device, ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        w, h, F = r["width"], r["height"], r["factor"]
        for kind in GUIDE_SETS:
            d, l = (next(c for c in r["calls"] if c["guides"] == kind and c["form"] == f) for f in ("direct", "lds"))
            print(f"| {-(-w // F)} x {-(-h // F)} -> {w} x {h} | {F} | {r['tiles']} | {kind} | {d['ms']:.4f} ({d['min_ms']:.4f}) | {l['ms']:.4f} ({l['min_ms']:.4f}) | "
                  f"{d['bytes'] / 1e6:.1f} | {max(d['gb_per_s'], l['gb_per_s']):.1f} | {r['denoise_ms']:.4f} ({r['denoise_min_ms']:.4f}) |")
    live = []
    for k in (1, 8):
        runs = {False: [], True: []}
        for _ in range(args.live_reps):
            for upsampled in (False, True):
                runs[upsampled].append(live_fps(rt, k, upsampled))
        live.append(dict(k=k, frames=LIVE_FRAMES, full=[round(v, 1) for v in runs[False]], upsampled=[round(v, 1) for v in runs[True]]))
    print(f"(rtrace -l --live-denoise, random balls 1200 x 800, depth 50, {LIVE_FRAMES} displayed frames of K samples per pixel; frames per second over the "
          f"live loop's own time — scene upload, guide renders and downloads included; median of {args.live_reps} sessions, their range in brackets)")
    print("| K | full size, fps | --upsample 2 --upsample-albedo --upsample-edges, fps | ratio of the medians |")
    print("|---|---|---|---|")
    for r in live:
        a, b = statistics.median(r["full"]), statistics.median(r["upsampled"])
        print(f"| {r['k']} | {a:.1f} ({min(r['full']):.1f} - {max(r['full']):.1f}) | {b:.1f} ({min(r['upsampled']):.1f} - {max(r['upsampled']):.1f}) | {b / a:.2f} |")
    print(json.dumps(dict(tool="upsample_speed", live=live, device=torch.cuda.get_device_name(0), repeats=args.repeats, rows=rows)))


if __name__ == "__main__":
    main()
